"""Constructed windows for pgorb_local_bundle_adjustment (pilotguru_amd/csrc/local_ba.hip) and the runners that put them through the
plain reference (tests/lba_reference.py), the single call and the batched device form.  A helper module (no tests);
tests/test_local_bundle_adjustment.py and tests/golden/make_lba_spread.py use it.

Every scene has pixel noise and a few far points.  The noise keeps the optimum's chi2 macroscopic, the far points (low parallax, so
lambda governs them for several iterations) keep every iteration's improvement far above the rounding of the chi2 sum: Levenberg's
decisions then stay away from their thresholds (the case condition, `condition`), which a noise-free scene converged to the last bit
cannot offer."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_reference as LR  # noqa: E402
import pose_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
NLEVELS = 8
INV_SIGMA2 = PR.inv_level_sigma2(1.2, NLEVELS)
SIGMA = 1.0 / np.sqrt(INV_SIGMA2.astype(f64))
CAM_A = (520.0, 515.0, 320.0, 240.0)
CAM_B = (610.0, 600.0, 350.5, 255.25)
POSE_SENTINEL = 0x5A
SPREAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lba_spread.json")


def se3_matrix(E):
    return np.concatenate([PR.matrix_from_quat(E.q), E.t.reshape(3, 1)], 1)


def camera_at(rng, centre, tilt=0.05):
    """A camera at `centre` looking down +z, tilted by a small random rotation: its SE3 (world to camera)."""
    E = PR.se3_exp(np.concatenate([rng.normal(0, tilt, 3), np.zeros(3)]))
    R = PR.matrix_from_quat(E.q)
    return PR.SE3(E.q, -R @ np.asarray(centre, f64))


class Builder:
    """Frames, points and observations, one at a time; problem() lays them out as the interface takes them."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.true_T, self.in_T, self.cam, self.bad = [], [], [], []
        self.keys, self.octs, self.slots = [], [], []
        self.X_true, self.X_in, self.pbad, self.obs = [], [], [], []

    def add_camera(self, centre, cam=CAM_A, twist=None, bad=False, tilt=0.05):
        E = camera_at(self.rng, centre, tilt)
        start = E if twist is None else PR.oplus(E, np.concatenate([self.rng.normal(0, twist[0], 3), self.rng.normal(0, twist[1], 3)]))
        self.true_T.append(E)
        self.in_T.append(PR.to_pose_floats(start)[0])
        self.cam.append(cam)
        self.bad.append(int(bad))
        self.keys.append([])
        self.octs.append([])
        self.slots.append([])
        return len(self.true_T) - 1

    def add_point(self, X, jitter=0.05, bad=False, start=None):
        self.X_true.append(np.asarray(X, f64))
        self.X_in.append(np.asarray(X, f64) + self.rng.normal(0, jitter, 3) if start is None else np.asarray(start, f64))
        self.pbad.append(int(bad))
        self.obs.append([])
        return len(self.X_true) - 1

    def project(self, f, X):
        T, (fx, fy, cx, cy) = se3_matrix(self.true_T[f]), self.cam[f]
        pc = T[:, :3] @ np.asarray(X, f64) + T[:, 3]
        return np.array([pc[0] / pc[2] * fx + cx, pc[1] / pc[2] * fy + cy]), pc[2]

    def add_key(self, f, xy, octave, slot=-1):
        self.keys[f].append(np.asarray(xy, f32))
        self.octs[f].append(int(octave))
        self.slots[f].append(int(slot))
        return len(self.keys[f]) - 1

    def observe(self, p, f, noise=0.7, octave=None, offset=None, slot=True, listed=True, xy=None):
        """Point p seen in frame f: a keypoint at its projection plus noise (in sigmas of its level) plus `offset` pixels; `slot`: the
        key frame's slot names the point, `listed`: the point's observation list names the key frame."""
        o = int(self.rng.integers(0, NLEVELS)) if octave is None else octave
        if xy is None:
            xy, _ = self.project(f, self.X_true[p])
            xy = xy + self.rng.normal(0, noise, 2) * SIGMA[o] + (0 if offset is None else np.asarray(offset, f64))
        i = self.add_key(f, xy, o, p if slot else -1)
        if listed:
            self.obs[p].append((f, i))
        return i

    def problem(self, local_kf, id0=None, name="", extra_keys=0):
        nf = len(self.keys)
        for f in range(nf):                                     # keypoints no point owns
            for _ in range(extra_keys):
                self.add_key(f, self.rng.uniform(0, 600, 2), self.rng.integers(0, NLEVELS))
        start, fr, ix = [0], [], []
        for lst in self.obs:
            for f, i in sorted(lst):
                fr.append(f)
                ix.append(i)
            start.append(len(fr))
        fixed = np.zeros(nf, np.uint8)
        if id0 is not None:
            fixed[id0] = 1
        P = LR.Problem([np.array(k, f32).reshape(-1, 2) for k in self.keys], self.octs, np.array(self.in_T, f32), np.array(self.cam, f32),
                       self.bad, self.slots, fixed, local_kf, np.array(self.X_in, f64).astype(f32).reshape(-1, 3), self.pbad, start, fr, ix,
                       INV_SIGMA2, name)
        P.true_T, P.true_X = [se3_matrix(E) for E in self.true_T], np.array(self.X_true, f64)      # what generated the observations
        return P


def window(name, seed, nlocal, nfixed, npts, nobs=3, noise=0.7, outliers=0, far=3, id0=None, edges=None, twist=(0.004, 0.02), extra=None,
           two_cams=False):
    """The standard scene: cameras on a line looking at a box of points, `nobs` observations a point (the first in a local key frame),
    `far` low-parallax points, `outliers` gross observations; `edges` trims or pads the observation count; extra(B, local, fixed) adds more."""
    B = Builder(seed)
    rng = B.rng
    ncam = nlocal + nfixed
    xs = np.linspace(-1.5, 1.5, ncam) if ncam > 1 else np.array([0.0])
    order = rng.permutation(ncam)                              # local and fixed cameras interleaved along the line
    cams = [None] * ncam
    for j, c in enumerate(order):
        is_local = j < nlocal
        cams[j] = B.add_camera([xs[c], rng.normal(0, 0.1), rng.normal(0, 0.1)], CAM_B if (two_cams and c % 2) else CAM_A,
                               twist if is_local and j != id0 else None)
    local, fixed = list(range(nlocal)), list(range(nlocal, ncam))
    pending = []
    for k in range(npts):
        isfar = k < far
        X = [rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(40, 60) if isfar else rng.uniform(4, 9)]
        p = B.add_point(X, 0.5 if isfar else 0.04)
        seen = [int(rng.choice(local))]
        others = [c for c in range(ncam) if c != seen[0]]
        seen += [int(c) for c in rng.choice(others, min(nobs - 1, len(others)), replace=False)]
        for f in seen:
            pending.append((p, f))
    if edges is not None:                                       # the exact count: drop observations of points seen 3 times, or add some
        while len(pending) > edges:
            counts = {}
            for p, f in pending:
                counts[p] = counts.get(p, 0) + 1
            cand = [i for i, (p, f) in enumerate(pending) if counts[p] >= 3 and (i == 0 or pending[i - 1][0] == p)]
            pending.pop(cand[int(rng.integers(len(cand)))])
        while len(pending) < edges:
            p = int(rng.integers(npts))
            free = [c for c in range(ncam) if (p, c) not in pending]
            if free:
                pending.append((p, int(rng.choice(free))))
    bad_ones = set(int(i) for i in rng.choice(len(pending), outliers, replace=False)) if outliers else set()
    for i, (p, f) in enumerate(pending):
        off = None
        if i in bad_ones:
            a = rng.uniform(0, 2 * np.pi)
            off = np.array([np.cos(a), np.sin(a)]) * rng.uniform(25, 60)
        B.observe(p, f, noise, offset=off)
    if extra is not None:
        extra(B, local, fixed)
    return B.problem(local, id0, name, extra_keys=2)


# ---------------------------------------------------------------- the structure case
def _structure(B, local, fixed):
    rng = B.rng
    # one point seen once: Hll has rank 2 and only lambda makes it invertible
    p = B.add_point([0.3, -0.2, 6.0])
    B.observe(p, local[0])
    # one point all of whose edges go to level 1: it lies BEHIND its cameras, where its observations agree with it (a point can
    # always move to satisfy one gross observation, so chi2 alone cannot set all of a point's edges aside; the depth can)
    p = B.add_point([-0.6, 0.4, -5.0])
    for f in (local[1], fixed[0], fixed[1]):
        B.observe(p, f)
    # a local key frame that loses all its level-0 edges, for the same reason: it looks the other way (a half turn about y), so
    # every point it lists is behind it
    c = np.array([0.2, 0.6, 0.1])
    lone = B.add_camera(c)
    B.true_T[lone] = PR.SE3([0.0, 1.0, 0.0, 0.0], [c[0], -c[1], c[2]])
    B.in_T[lone] = PR.to_pose_floats(PR.oplus(B.true_T[lone], np.concatenate([rng.normal(0, 0.004, 3), rng.normal(0, 0.02, 3)])))[0]
    local.append(lone)
    for q in rng.choice(np.arange(3, 12), 4, replace=False):
        B.observe(int(q), lone)
    # bad points in slots, a bad frame in observation lists, a bad key frame named by the window
    p = B.add_point([0.9, 0.1, 7.0], bad=True)
    B.observe(p, local[0])
    B.observe(p, fixed[0])
    badf = B.add_camera([0.0, -0.5, 0.0], bad=True)
    for q in rng.choice(np.arange(3, 12), 4, replace=False):
        B.observe(int(q), badf)
    badl = B.add_camera([0.4, -0.6, 0.0], bad=True)
    local.append(badl)
    for q in rng.choice(np.arange(3, 12), 3, replace=False):
        B.observe(int(q), badl)
    # slots and lists that disagree: a slot whose point does not list the key frame (local, but no edge there), and a listed
    # observation whose slot is empty; the first makes a point local that nothing else would
    p = B.add_point([-1.0, -0.5, 8.0])
    B.observe(p, local[0], listed=False)
    B.observe(p, fixed[0], slot=False)
    B.observe(p, fixed[1], slot=False)
    # a point so near that its Hll holds the largest diagonal entry (computeLambdaInit runs over all vertices)
    p = B.add_point([0.05, 0.02, 0.35], jitter=0.002)
    for j, f in enumerate([local[0], fixed[0], fixed[1]]):
        B.observe(p, f, octave=j)


def _depth_survivor(B, local, fixed):
    """Reading 7.  P is held by two fixed cameras 0.06 apart (its depth along their common ray is weak, so while lambda is large
    Levenberg walks it slowly) and starts 2 behind where it belongs.  The fixed camera A lies ON that ray between the start and the
    goal and sees P at the pixel every point of the ray has: A's chi2 is small wherever P is, its depth negative until P has walked
    past.  The first optimize ends with P still behind A -- A's edge is set aside for depth alone --, the second brings P in front:
    the edge keeps its small round-1 chi2 and survives.  (P is local through a slot its list does not name.)"""
    c1 = np.array([0.1, 0.3, -0.2])
    F1, F2 = B.add_camera(c1, tilt=0.0), B.add_camera(c1 + np.array([0.06, 0.0, 0.0]), tilt=0.0)
    d = np.array([0.05, -0.03, 1.0])
    d = d / np.linalg.norm(d)
    A = B.add_camera(c1 + 8.6 * d, tilt=0.0)
    p = B.add_point(c1 + 9.0 * d, start=c1 + 7.0 * d)
    B.observe(p, local[0], listed=False)
    B.observe(p, F1, noise=0.0, octave=0, slot=False)
    B.observe(p, F2, noise=0.0, octave=0, slot=False)
    xyA, _ = B.project(A, c1 + 9.0 * d)
    B.observe(p, A, xy=xyA, octave=0, slot=False)


CASE_NAMES = ["kf1", "kf2", "kf10", "kf11", "edges63", "edges64", "edges65", "edges257", "points257", "no_gauge", "id0_local",
              "structure", "outliers", "rounds1", "depth_survivor", "exact_optimum"]


def exact_optimum():
    """Every quantity binary-exact and every residual 0: identity rotations, dyadic centres, points and intrinsics, so b = 0, the
    update is 0, tempChi == currentChi and rho == 0: Terminate on a rejected trial, nothing changes."""
    keys, octs, slots, T = [[], [], []], [[], [], []], [[], [], []], []
    centres = [(-0.5, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)]
    cam = (512.0, 512.0, 320.0, 240.0)
    pts = [(x * 0.5, y * 0.5, 4.0) for x in (-1, 0, 1) for y in (-1, 0, 1)]
    start, fr, ix = [0], [], []
    for c in centres:
        T.append(np.array([[1, 0, 0, -c[0]], [0, 1, 0, -c[1]], [0, 0, 1, -c[2]]], f32))
    for p, X in enumerate(pts):
        for f, c in enumerate(centres):
            x, y, z = X[0] - c[0], X[1] - c[1], X[2] - c[2]
            keys[f].append((x / z * cam[0] + cam[2], y / z * cam[1] + cam[3]))
            octs[f].append(p % NLEVELS)
            slots[f].append(p)
            fr.append(f)
            ix.append(len(keys[f]) - 1)
        start.append(len(fr))
    return LR.Problem(keys, octs, T, [cam] * 3, [0, 0, 0], slots, [0, 0, 0], [0, 1], pts, [0] * len(pts), start, fr, ix, INV_SIGMA2, "exact_optimum")


def make_case(name):
    """(problem, rounds)"""
    if name == "kf1":
        return window(name, 101, 1, 2, 14), 2
    if name == "kf2":
        return window(name, 102, 2, 2, 18), 2
    if name == "kf10":
        return window(name, 110, 10, 3, 40), 2
    if name == "kf11":
        return window(name, 111, 11, 2, 44), 2
    if name.startswith("edges"):
        n = int(name[5:])
        return window(name, 200 + n, 3, 2, max(21, n // 3), edges=n, outliers=2), 2
    if name == "points257":
        return window(name, 257, 4, 2, 257, nobs=3, outliers=8), 2
    if name == "no_gauge":
        return window(name, 301, 3, 0, 24, nobs=3), 2
    if name == "id0_local":
        return window(name, 302, 3, 1, 24, id0=1, outliers=2), 2
    if name == "structure":
        return window(name, 401, 3, 2, 30, extra=_structure, two_cams=True, outliers=2), 2
    if name == "outliers":
        return window(name, 503, 4, 3, 60, nobs=4, outliers=20, noise=1.0), 2
    if name == "rounds1":
        return window(name, 503, 4, 3, 60, nobs=4, outliers=20, noise=1.0), 1
    if name == "depth_survivor":
        return window(name, 601, 2, 2, 20, noise=0.02, far=0, extra=_depth_survivor), 2
    if name == "exact_optimum":
        return exact_optimum(), 2
    raise KeyError(name)


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]


def all_cases():
    return [(n,) + case(n) for n in CASE_NAMES]


_ref_cache = {}


def run_reference(name, rules=LR.REFERENCE, form=LR.Form()):
    key = (name, rules, form)
    if key not in _ref_cache:
        P, rounds = case(name)
        _ref_cache[key] = LR.local_bundle_adjustment(P, rounds, rules, form)
    return _ref_cache[key]


# ---------------------------------------------------------------- tolerances (tests/golden/lba_spread.json)
FLOAT_OUTPUTS = ("R", "t", "Ow", "pos", "chi2")
DECISIONS = ("chi2", "depth", "rho", "stop", "pivot")
INT_OUTPUTS = ("ret", "erase", "level", "is_local", "role", "info")
ULP1 = float(np.spacing(f32(1.0)))


def scaled_differences(P, a, b):
    """The largest difference per float output between two results over the local key frames and local points: rotation entries
    as they are, tcw, Ow and pos over max(1, |.|inf) of the vector, chi2 over max(1, chi2)."""
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    if a["info"][0] or b["info"][0]:
        return out
    for f in np.flatnonzero(a["role"] == LR.ROLE_LOCAL):
        Ta, Tb = a["pose_Tcw"][f].astype(f64).reshape(3, 4), b["pose_Tcw"][f].astype(f64).reshape(3, 4)
        out["R"] = max(out["R"], float(np.abs(Ta[:, :3] - Tb[:, :3]).max()))
        out["t"] = max(out["t"], float(np.abs(Ta[:, 3] - Tb[:, 3]).max()) / max(1.0, float(np.abs(Ta[:, 3]).max())))
        oa, ob = a["pose_Ow"][f].astype(f64), b["pose_Ow"][f].astype(f64)
        out["Ow"] = max(out["Ow"], float(np.abs(oa - ob).max()) / max(1.0, float(np.abs(oa).max())))
    pa, pb = a["pos"].astype(f64), b["pos"].astype(f64)
    if len(pa):
        out["pos"] = float((np.abs(pa - pb).max(1) / np.maximum(1.0, np.abs(pa).max(1))).max())
    ca, cb = a["chi2"].astype(f64), b["chi2"].astype(f64)
    if len(ca):
        out["chi2"] = float((np.abs(ca - cb) / np.maximum(1.0, np.abs(ca))).max())
    return out


def spread(name):
    """Per float output the largest scaled difference between any two of the reference's arithmetic forms (the outputs are floats:
    it is 0 where the forms round to the same float), and per decision quantity (the chi2 and depth nearest their thresholds, the
    smallest |rho|, the 1e3 rule's and the pivots' margins: relative, in double) the largest difference between the forms."""
    P, _ = case(name)
    rs = [run_reference(name, form=fm) for fm in LR.FORMS]
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for i in range(len(rs)):
        for j in range(i + 1, len(rs)):
            d = scaled_differences(P, rs[i], rs[j])
            out = {k: max(out[k], d[k]) for k in out}
    for k in DECISIONS:                                         # the decision quantities in double, where the forms do differ
        v = [r["margins"][k] for r in rs if k in r["margins"] and np.isfinite(r["margins"][k])]
        out["decision_" + k] = float(max(v) - min(v)) if v else 0.0
    return out


def recorded_spread():
    with open(SPREAD_FILE) as f:
        return json.load(f)["spread"]


def bounds(recorded):
    """The bound per output: the larger of 2 float ulps at the output's scale (the differences are scaled to 1) and 16 x the recorded
    spread.  The floor is there because the outputs are rounded to float: two doubles 1e-12 apart can land on neighbouring floats."""
    return {k: max(2.0 * ULP1, 16.0 * float(recorded[k])) for k in FLOAT_OUTPUTS}


def window_of(recorded, decision=None):
    """The case condition's window: no decision may lie nearer its threshold (relatively) than 16 x the largest recorded spread of
    the case's outputs, nor than 16 x the recorded spread of that decision quantity between the forms, and never nearer than 1e-9."""
    w = max(1e-9, 16.0 * max(float(recorded[k]) for k in FLOAT_OUTPUTS))
    return w if decision is None else max(w, 16.0 * float(recorded.get("decision_" + decision, 0.0)))


def condition(name, recorded, forms=None):
    """What breaks the case condition under any form: a chi2 at a classification near 5.991, a depth near 0, a Levenberg decision
    (rho's sign, the 1e3 rule, a pivot's sign) near its threshold, or integer outputs that differ between the forms."""
    base = run_reference(name)
    bad = []
    for fm in (LR.FORMS if forms is None else forms):
        r = run_reference(name, form=fm)
        m = r["margins"]
        for k in DECISIONS:
            w = window_of(recorded, k)
            lim = {"depth": max(w, 1e-3), "stop": 1e3 * w}.get(k, w)
            if k in m and not m[k] > lim:
                bad.append("%s under %s: %s margin %.3g <= %.3g" % (name, fm, k, m[k], lim))
        for k in INT_OUTPUTS:
            if not np.array_equal(r[k], base[k]):
                bad.append("%s under %s: %s differs from the default form" % (name, fm, k))
    return bad


def differences(P, want, got, recorded):
    """The compared outputs that differ: integers and flags exactly; with a status the poses and points as bytes; floats by bounds()."""
    bad = [k for k in INT_OUTPUTS if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    if want["info"][0]:
        if want["pos"].tobytes() != got["pos"].tobytes():
            bad.append("pos bytes")
        if got["chi2"].any():
            bad.append("chi2")
        return bad
    d, b = scaled_differences(P, want, got), bounds(recorded)
    return bad + ["%s %.3g > %.3g" % (k, d[k], b[k]) for k in FLOAT_OUTPUTS if not d[k] <= b[k]]


# ---------------------------------------------------------------- GPU runners
def keypoints(keys_xy, octaves):
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(len(octaves), KEYPOINT_DTYPE)
    if len(octaves):
        k["x"], k["y"], k["octave"] = keys_xy[:, 0], keys_xy[:, 1], octaves
    return k


def pose_records(P):
    from pilotguru_amd.orb import KF_POSE_DTYPE, kf_pose
    out = np.zeros(P.nframes, KF_POSE_DTYPE)
    for f in range(P.nframes):
        out[f] = kf_pose(P.Tcw[f].reshape(3, 4), PR.to_pose_floats(PR.to_se3(P.Tcw[f]))[1], *P.cam[f])
    return out


def table(P):
    from pilotguru_amd.orb import MAP_POINT_DTYPE
    pts = np.zeros(len(P.pos), MAP_POINT_DTYPE)
    pts["pos"] = P.pos
    pts["normal"], pts["min_distance"], pts["max_distance"] = 0.25, 1.5, 9.5      # must keep their bytes
    return pts


def other_bytes(pts):
    """The bytes of the fields the adjustment must leave alone."""
    pts = np.asarray(pts)
    return pts["normal"].tobytes() + pts["min_distance"].tobytes() + pts["max_distance"].tobytes()


def result_of(P, poses_in, pose_out, pts, erase, chi2, level, is_local, role, info, ret):
    role = np.asarray(role, np.uint8)
    loc = role == LR.ROLE_LOCAL
    return dict(ret=int(ret), pose_Tcw=np.array(pose_out["Tcw"], f32), pose_Ow=np.array(pose_out["Ow"], f32), pos=np.array(pts["pos"], f32),
                erase=np.asarray(erase, np.uint8), chi2=np.asarray(chi2, f32), level=np.asarray(level, np.uint8),
                is_local=np.asarray(is_local, np.uint8), role=role, info=np.asarray(info, np.int32),
                pose_bytes=np.asarray(pose_out)[loc].tobytes(), pose_in_bytes=np.asarray(poses_in)[loc].tobytes(),
                pose_rest_bytes=np.asarray(pose_out)[~loc].tobytes(), pose_in_rest_bytes=np.asarray(poses_in)[~loc].tobytes(),
                other_bytes=other_bytes(pts), table_bytes=np.asarray(pts).tobytes())


def run_gpu(P, rounds, ext):
    """The single call through the C ABI; a negative return value comes back as it is."""
    from pilotguru_amd.orb import KF_POSE_DTYPE
    L, h = ext._L, ext._h
    nf, npts, nobs = P.nframes, len(P.pos), len(P.obs_frame)
    ks = [keypoints(P.keys_xy[f], P.octaves[f]) for f in range(nf)]
    sl = [np.ascontiguousarray(s, np.int32) for s in P.kf_point]
    kps, slots = (C.c_void_p * max(nf, 1))(), (C.c_void_p * max(nf, 1))()
    for f in range(nf):
        kps[f], slots[f] = ks[f].ctypes.data, sl[f].ctypes.data
    n = np.array([len(o) for o in P.octaves], np.int32)
    poses, pts = pose_records(P), table(P)
    out = np.zeros(max(nf, 1), KF_POSE_DTYPE)
    er, lv, chi = np.full(max(nobs, 1), 9, np.uint8), np.full(max(nobs, 1), 9, np.uint8), np.full(max(nobs, 1), -9, f32)
    il, ro, info = np.full(max(npts, 1), 9, np.uint8), np.full(max(nf, 1), 9, np.uint8), np.full(LR.INFO, -9, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ret = L.pgorb_local_bundle_adjustment(h, nf, kps, p(n), p(poses), p(P.kf_bad), slots, p(P.fixed_id0), len(P.local_kf), p(P.local_kf), npts,
                                          p(pts), p(P.point_bad), p(P.obs_start), p(P.obs_frame), p(P.obs_idx), rounds, p(out), p(er), p(chi),
                                          p(lv), p(il), p(ro), p(info))
    if ret < 0:
        return ret
    return result_of(P, poses, out[:nf], pts, er[:nobs], chi[:nobs], lv[:nobs], il[:npts], ro[:nf], info, ret)


class Batch:
    """Several windows over one batch of frames and one table: the problems side by side, frames and points renumbered."""

    def __init__(self, names, cap_extra=5):
        self.names = list(names)
        self.problems = [case(n)[0] for n in self.names]
        self.rounds = case(self.names[0])[1]
        self.f0 = np.cumsum([0] + [P.nframes for P in self.problems])
        self.p0 = np.cumsum([0] + [len(P.pos) for P in self.problems])
        self.o0 = np.cumsum([0] + [len(P.obs_frame) for P in self.problems])
        self.cap = max(max(len(o) for o in P.octaves) for P in self.problems) + cap_extra
        if self.cap % 64 == 0:
            self.cap += 1


def run_gpu_batch(b, ext, order=None, stream=None, refresh=None, time_reps=0):
    """One call of pgorb_local_bundle_adjustment_batch_device over the windows in `order`; the per-window results in that order.
    refresh = (ref_obs per problem): chains pgorb_refresh_map_points_batch_device (normal and depth, the local points) on the same
    resident arrays and returns the table it leaves as well."""
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE, Optimizer, MP_NORMAL_DEPTH
    order = list(range(len(b.problems))) if order is None else list(order)
    nf, npts, nobs, cap = int(b.f0[-1]), int(b.p0[-1]), int(b.o0[-1]), b.cap
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["octave"] = np.nan, np.nan, 99                 # past n: never read
    slots = np.full((nf, cap), 12345678, np.int32)
    n = np.zeros(nf, np.int32)
    poses, pts = np.zeros(nf, KF_POSE_DTYPE), np.zeros(npts, MAP_POINT_DTYPE)
    kf_bad, id0, pbad = np.zeros(nf, np.uint8), np.zeros(nf, np.uint8), np.zeros(npts, np.uint8)
    ostart, ofr, oix = np.zeros(npts + 1, np.int32), np.zeros(nobs, np.int32), np.zeros(nobs, np.int32)
    for j, P in enumerate(b.problems):
        f0, p0, o0 = int(b.f0[j]), int(b.p0[j]), int(b.o0[j])
        for f in range(P.nframes):
            m = len(P.octaves[f])
            kp[f0 + f, :m] = keypoints(P.keys_xy[f], P.octaves[f])
            slots[f0 + f, :m] = np.where(P.kf_point[f] >= 0, P.kf_point[f] + p0, -1)
            n[f0 + f] = m
        poses[f0:f0 + P.nframes], pts[p0:p0 + len(P.pos)] = pose_records(P), table(P)
        kf_bad[f0:f0 + P.nframes], id0[f0:f0 + P.nframes], pbad[p0:p0 + len(P.pos)] = P.kf_bad, P.fixed_id0, P.point_bad
        ostart[p0 + 1:p0 + len(P.pos) + 1] = P.obs_start[1:] + o0
        ofr[o0:o0 + len(P.obs_frame)], oix[o0:o0 + len(P.obs_frame)] = P.obs_frame + f0, P.obs_idx
    ws, wk = [0], []
    for j in order:
        wk += [int(f) + int(b.f0[j]) for f in b.problems[j].local_kf]
        ws.append(len(wk))
    st = torch.cuda.current_stream() if stream is None else stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.cuda.stream(st):
        d_kps, d_n, d_pose = dev(kp.view(np.uint8).reshape(nf, cap, KEYPOINT_DTYPE.itemsize)), dev(n), dev(poses.view(np.uint8).reshape(nf, -1))
        d_slots, d_pts = dev(slots), dev(pts.view(np.uint8).reshape(npts, -1))
        d_os, d_of, d_oi = dev(ostart), dev(ofr), dev(oix)
        # pose_out is written for local key frames only: the other rows keep a sentinel (the refresh needs real poses there: a copy)
        sentinel = None if refresh is not None else torch.full_like(d_pose, POSE_SENTINEL)
        d_ws, d_wk, d_pb, d_kb, d_id = dev(np.array(ws, np.int32)), dev(np.array(wk, np.int32)), dev(pbad), dev(kf_bad), dev(id0)
        call = lambda: Optimizer.LocalBundleAdjustment_batch_device(ext, d_kps, d_n, cap, d_pose, d_slots, d_ws, d_wk, npts, d_pts, d_os, d_of, d_oi,
                                                                    d_pb, d_kb, d_id, b.rounds, d_pose_out=sentinel, stream=st.cuda_stream)
        if time_reps:                                           # HIP events around the call alone; the points are put back before each
            start_pts, ms = d_pts.clone(), []
            for _ in range(time_reps + 1):
                d_pts.copy_(start_pts)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                st.synchronize()
                ms.append(e0.elapsed_time(e1))
            b.ms = float(np.median(ms[1:]))
            d_pts.copy_(start_pts)
        out = call()
        refreshed = None
        if refresh is not None:
            ref_obs = np.zeros(npts, np.int32)
            for j, r in enumerate(refresh):
                ref_obs[int(b.p0[j]):int(b.p0[j + 1])] = r
            sel = torch.nonzero(out["is_local"].sum(0)).to(torch.int32).reshape(-1).contiguous()
            status = torch.zeros(max(int(sel.numel()), 1), dtype=torch.int32, device="cuda")
            d_desc = torch.zeros((nf, cap, 32), dtype=torch.uint8, device="cuda")
            d_pd = torch.zeros((npts, 32), dtype=torch.uint8, device="cuda")
            q = lambda t: C.c_void_p(t.data_ptr())
            ext._check(ext._L.pgorb_refresh_map_points_batch_device(
                ext._h, q(d_kps), q(d_desc), q(d_n), nf, cap, q(out["pose_out"]), q(dev(kf_bad)), npts, q(d_pts), q(d_pd), q(dev(pbad)), q(d_os),
                q(d_of), q(d_oi), nobs, q(dev(ref_obs)), int(sel.numel()), q(sel), MP_NORMAL_DEPTH, None, q(status), C.c_void_p(st.cuda_stream)))
            refreshed = True
    st.synchronize()
    po = np.frombuffer(out["pose_out"].cpu().numpy().tobytes(), KF_POSE_DTYPE)
    tb = np.frombuffer(d_pts.cpu().numpy().tobytes(), MAP_POINT_DTYPE)
    er, chi, lv, il, ro, info, ne = (out[k].cpu().numpy() for k in ("erase", "chi2", "level", "is_local", "role", "info", "nerased"))
    res = []
    for w, j in enumerate(order):
        P = b.problems[j]
        f, p, o = slice(int(b.f0[j]), int(b.f0[j + 1])), slice(int(b.p0[j]), int(b.p0[j + 1])), slice(int(b.o0[j]), int(b.o0[j + 1]))
        r = result_of(P, poses[f], po[f], tb[p], er[w, o], chi[w, o], lv[w, o], il[w, p], ro[w, f], info[w], ne[w])
        outside = np.ones(nobs, bool)
        outside[o] = False
        outp, outf = np.ones(npts, bool), np.ones(nf, bool)
        outp[p], outf[f] = False, False
        r["elsewhere_zero"] = bool(not er[w, outside].any() and not chi[w, outside].any() and not lv[w, outside].any() and
                                   not il[w, outp].any() and not ro[w, outf].any())
        res.append(r)
    if refreshed:
        return res, tb
    return res
