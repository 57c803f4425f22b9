"""Constructed scenes for the tracking thread's matchers with the projection on the device (pilotguru_amd/csrc/track.hip) and the
runners that put them through the plain reference (tests/tracking_reference.py), the single calls and the batched device forms.
A helper module (no tests): tests/test_tracking_projection.py uses it.

Keypoints are placed directly, no extraction.  The camera has fx = fy = 256 and its principal point at the origin of the image
coordinates, so the Frame's bounds are (-320, 320, -240, 240): a 640 x 480 frame whose four bounds are non-zero floats, which a
projection can meet exactly and miss by exactly one ulp.  The edge scenes use the identity pose (translation -0.0, so that a
camera-space z of -0.0 exists); the generic scenes use rotated and translated poses."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_cases as MC  # noqa: E402
import tracking_reference as TR  # noqa: E402
from matcher_cases import SF, ArrayFrame, at_distance, keys, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE, kf_pose  # noqa: E402

f32 = np.float32
NLEVELS = 8
FX = 256.0
BOUNDS = (-320.0, 320.0, -240.0, 240.0)
EDGE_POSE = kf_pose([[1, 0, 0, -0.0], [0, 1, 0, -0.0], [0, 0, 1, -0.0]], (0, 0, 0), FX, FX, 0.0, 0.0)
UP, DOWN = f32(np.inf), f32(-np.inf)


def log_sf():
    return f32(TR._LOG_F()(SF[1]))


def generic_pose(k):
    """Rotated about all three axes and off the origin."""
    return MC.pose(MC.rot(0.05 + 0.02 * k, -0.04 + 0.03 * k, 0.3 * k), (0.3 * k, -0.2, 0.1 * k), FX, 0.0, 0.0)


def axis_pose():
    """Axis-aligned: a quarter turn about the optical axis, the centre at (1, 2, -1)."""
    return MC.pose([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], (1.0, 2.0, -1.0), FX, 0.0, 0.0)


def pt(pos, normal=(0, 0, 1), min_d=1.0, max_d=16.0, bad=False, has_obs=True, desc=None):
    return dict(pos=np.asarray(pos, np.float32), normal=np.asarray(normal, np.float32), min_d=f32(min_d), max_d=f32(max_d),
                bad=bad, has_obs=has_obs, desc=desc)


class Case:
    """kind "local": slots (table index per keypoint or -1), queries, query_seen.  kind "last" / "kf": other_keys (the last frame's /
    key frame's keypoints), other_point (table index per such keypoint or -1), flag (last_outlier / already_found), has
    (kp_has_point).  points: the table, dicts of pt()."""

    def __init__(self, kind, name, k, d, pose, points, th, **kw):
        self.kind, self.name, self.keys, self.desc, self.pose, self.points, self.th = kind, name, k, d, pose, points, float(th)
        self.slots = kw.get("slots")
        self.queries = np.asarray(kw.get("queries", []), np.int32)
        self.query_seen = kw.get("query_seen")
        self.other_keys = kw.get("other_keys")
        self.other_point = None if kw.get("other_point") is None else np.asarray(kw["other_point"], np.int32)
        self.flag, self.has = kw.get("flag"), kw.get("has")
        self.orb_dist, self.ori, self.nnratio = kw.get("orb_dist", 100), kw.get("ori", True), 0.8

    def build(self):
        fr = TR.Frame(1, self.keys, self.desc, BOUNDS, self.pose, SF, log_sf(), NLEVELS)
        mps = [TR.MapPoint(i, p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"], p["bad"], p["has_obs"])
               for i, p in enumerate(self.points)]
        if self.slots is not None:
            fr.slots = [None if s < 0 else mps[s] for s in self.slots]
        return fr, mps


def run_reference(c, rules=TR.REFERENCE, hits=None):
    fr, mps = c.build()
    if c.kind == "local":
        return TR.search_local_points(fr, [mps[q] for q in c.queries], c.query_seen, c.th, c.nnratio, 0.5, rules, hits)
    other = [None if s < 0 else mps[s] for s in c.other_point]
    if c.kind == "last":
        return TR.search_by_projection_last_frame(fr, c.other_keys, other, c.flag, c.has, c.th, c.ori, rules, hits)
    return TR.search_by_projection_keyframe(fr, c.other_keys, other, c.flag, c.has, c.th, c.orb_dist, c.ori, rules, hits)


INT_FIELDS = {"local": ("nmatches", "assigned", "in_view", "level", "kp_point_out", "n_to_match"),
              "last": ("nmatches", "assigned", "valid"), "kf": ("nmatches", "assigned")}
BIT_FIELDS = {"local": ("proj_x", "proj_y", "view_cos"), "last": ("u", "v"), "kf": ("u", "v", "dist3d")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differences(kind, want, got):
    """The compared outputs that differ: integers by value, floats as bit patterns."""
    out = [k for k in INT_FIELDS[kind] if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    return out + [k for k in BIT_FIELDS[kind] if not np.array_equal(bits(want[k]), bits(got[k]))]


def table_arrays(points):
    n = len(points)
    pts = np.zeros(n, MAP_POINT_DTYPE)
    for i, p in enumerate(points):
        pts[i] = (p["pos"], p["normal"], p["min_d"], p["max_d"])
    return (pts, np.array([p["desc"] for p in points], np.uint8).reshape(n, 32), np.array([p["bad"] for p in points], np.uint8),
            np.array([p["has_obs"] for p in points], np.uint8))


# ---------------------------------------------------------------- building scenes
def _finish_points(points, rng):
    for p in points:
        if p["desc"] is None:
            p["desc"] = rand_desc(rng)[0]
    return points


def _front(pose, p):
    """(u, v, dist, level) of a point under the reference's arithmetic, or None when it does not project inside the bounds."""
    fr = TR.Frame(0, keys([], []), np.zeros((0, 32), np.uint8), BOUNDS, pose, SF, log_sf(), NLEVELS)
    pc = TR.to_camera(pose, p["pos"])
    with np.errstate(all="ignore"):
        invz = f32(f32(1) / pc[2])
    u, v = TR.project(pose, pc, invz)
    if not TR.in_bounds(fr, u, v):
        return None
    _, dist = TR.dist_to_centre(pose, p["pos"])
    with np.errstate(all="ignore"):
        lvl = TR.predict_scale(p["max_d"], dist, log_sf(), NLEVELS, TR._LOG_F())
    return u, v, dist, lvl


def world_point(pose, u, v, z):
    """The world point that projects to (u, v) at camera depth z (double arithmetic; the reference re-projects it in float)."""
    T = np.asarray(pose["Tcw"], np.float64).reshape(3, 4)
    pc = np.array([u * z / FX, v * z / FX, z])
    return (T[:, :3].T @ (pc - T[:, 3])).astype(np.float32)


def generic_points(rng, pose, n):
    """Points in front of the camera over the whole image, a few outside it; normals around the viewing ray (some beyond the
    viewing-angle limit), depth ranges that put PredictScale on every level, a few outside their range, a few bad."""
    Ow = np.asarray(pose["Ow"], np.float64)
    out = []
    for i in range(n):
        u, v = rng.uniform(-340, 340), rng.uniform(-255, 255)
        z = rng.uniform(2.0, 8.0) * (-1 if i % 29 == 7 else 1)
        pos = world_point(pose, u, v, z)
        ray = pos.astype(np.float64) - Ow
        dist = np.linalg.norm(ray)
        nrm = ray / dist + rng.normal(0, 0.9 if i % 5 == 0 else 0.03, 3)
        nrm = nrm / np.linalg.norm(nrm) * rng.uniform(0.9, 1.0)
        lvl = i % (NLEVELS + 2)
        max_d = dist * float(SF[1]) ** (lvl - 0.5) * (0.6 if i % 31 == 3 else 1.0)
        out.append(pt(pos, nrm, max_d / float(SF[NLEVELS - 1]) * (1.4 if i % 37 == 5 else 1.0), max_d, bad=i % 23 == 11, has_obs=i % 7 != 2))
    return _finish_points(out, rng)


def keypoints_for(rng, pose, points, which, extra, jitter=1.0):
    """One keypoint near the projection of every point of `which` that projects inside the bounds, on its predicted level or the
    one below, with a descriptor 5 .. 70 bits from the point's; then `extra` keypoints anywhere.  Returns (keys, desc, owner) with
    owner[i] = the point keypoint i was made for, or -1."""
    xs, ys, octs, ds, owner = [], [], [], [], []
    for j in which:
        f = _front(pose, points[j])
        if f is None:
            continue
        u, v, _, lvl = f
        xs.append(min(max(float(u) + rng.uniform(-jitter, jitter), BOUNDS[0]), BOUNDS[1] - 0.01))
        ys.append(min(max(float(v) + rng.uniform(-jitter, jitter), BOUNDS[2]), BOUNDS[3] - 0.01))
        octs.append(max(lvl - int(rng.randint(0, 2)), 0))
        ds.append(at_distance(points[j]["desc"], int(rng.randint(5, 70)), rng))
        owner.append(j)
    for _ in range(extra):
        xs.append(rng.uniform(BOUNDS[0], BOUNDS[1] - 0.01)); ys.append(rng.uniform(BOUNDS[2], BOUNDS[3] - 0.01))
        octs.append(int(rng.randint(0, NLEVELS))); ds.append(rand_desc(rng)[0]); owner.append(-1)
    order = rng.permutation(len(xs))
    k = keys(np.array(xs)[order], np.array(ys)[order], octave=np.array(octs, np.int32)[order], angle=rng.uniform(0, 360, len(xs)).astype(np.float32))
    return k, np.array(ds, np.uint8).reshape(-1, 32)[order], np.array(owner, np.int32)[order]


def _bound_for(target, fac):
    """A float b with fac*b == target in float (the getters' 0.8f*mfMinDistance / 1.2f*mfMaxDistance)."""
    b = f32(f32(target) / f32(fac))
    for _ in range(8):
        for cand in (b, np.nextafter(b, UP), np.nextafter(b, DOWN)):
            if f32(f32(fac) * cand) == f32(target):
                return cand
        b = np.nextafter(b, UP)
    raise AssertionError("no float b with %r * b == %r" % (fac, target))


def bounds_points():
    """u and v exactly on each of the four bounds and one ulp outside: fx*X/4 = 64*X and 64*Y are exact."""
    out = []
    for x in (5.0, -5.0):
        out += [pt((x, 0, 4), (0, 0, 1)), pt((np.nextafter(f32(x), UP if x > 0 else DOWN), 0, 4), (0, 0, 1))]
    for y in (3.75, -3.75):
        out += [pt((0, y, 4), (0, 0, 1)), pt((0, np.nextafter(f32(y), UP if y > 0 else DOWN), 4), (0, 0, 1))]
    return out


def zero_depth_points():
    """PcZ of -0.0 (NaN and infinite projections), +0 (both), a tiny positive value, a negative value."""
    return [pt((-0.0, -0.0, -0.0)), pt((-1.0, -1.0, -0.0)), pt((0.0, 0.0, 0.0)), pt((1.0, 0.0, 0.0)),
            pt((2.0 ** -101, 0.0, 2.0 ** -100), min_d=0.0, max_d=1.0), pt((0.5, 0.25, -4.0))]


def depth_points():
    """On the optical axis dist = Z exactly: dist on 0.8f*min_distance and 1.2f*max_distance and one ulp either side.  At the far
    bound max_distance / dist is about 1 / 1.2, where PredictScale's quotient falls either side of -1 (the low clamp)."""
    out = []
    for z0 in (4.0, 4.5, 5.5):                                                  # (at 4.5 and 5.5 the quotient is below -1)
        mn, mx = _bound_for(z0, f32(0.8)), _bound_for(z0, f32(1.2))
        for z in (f32(z0), np.nextafter(f32(z0), DOWN), np.nextafter(f32(z0), UP)):
            out += [pt((0, 0, z), min_d=mn, max_d=16.0), pt((0, 0, z), min_d=1.0, max_d=mx)]
    return out


def local_edges():
    """The edge scene of SearchLocalPoints under the identity pose: see the functions above, then the viewing cosine on 0.5 and one
    ulp below, either side of 0.998, PredictScale clamped high, and the slot / seen rules."""
    rng = np.random.RandomState(11)
    P = zero_depth_points() + bounds_points() + depth_points()
    half = f32(0.5)
    P += [pt((0, 0, 4), (0, 0, half), 2, 8), pt((0, 0, 4), (0, 0, np.nextafter(half, DOWN)), 2, 8)]
    iA, iB = len(P), len(P) + 1
    P += [pt((0, 0, 4), (0, 0, f32(0.998)), 2, 8), pt((0, 0, 4), (0, 0, np.nextafter(f32(0.998), DOWN)), 2, 8)]
    P += [pt((0, 0, 4), min_d=1.0, max_d=4.0 * 1.2 ** 10)]                        # PredictScale above the last level
    iBad, iTaker, iSlotQ, iSeen, iBadQ, iSlotOnly = range(len(P), len(P) + 6)
    P += [pt((2, 1, 4), bad=True), pt((2, 1, 4), (0, 0, 1), 2, 8),                # a bad point in a slot; the query that takes its keypoint
          pt((-2, 1, 4), (0, 0, 1), 2, 8), pt((-2, -1, 4), (0, 0, 1), 2, 8),      # a slot's point that is also a query; query_seen
          pt((2, -1, 4), (0, 0, 1), 2, 8, bad=True), pt((1, 1, 4), (0, 0, 1), 2, 8, has_obs=False)]
    _finish_points(P, rng)
    queries = [i for i in range(len(P)) if i not in (iBad, iSlotOnly)]
    k, d, owner = keypoints_for(rng, EDGE_POSE, P, [i for i in queries if i not in (iA, iB)] + [iSlotOnly], 20)
    # either side of 0.998: the radius is 2.5 or 4 times sf[level]; a keypoint 6 px away lies between the two at level 4
    ka = keys([6.0, 0.0], [0.0, 6.0], octave=4)
    k = np.concatenate([k, ka])
    d = np.concatenate([d, np.array([at_distance(P[iA]["desc"], 5, rng), at_distance(P[iB]["desc"], 5, rng)], np.uint8)])
    owner = np.concatenate([owner, [iA, iB]])
    slots = np.full(len(k), -1, np.int32)
    slots[np.flatnonzero(owner == iTaker)[0]] = iBad
    slots[np.flatnonzero(owner == iSlotQ)[0]] = iSlotQ
    slots[np.flatnonzero(owner == iSlotOnly)[0]] = iSlotOnly
    seen = np.zeros(len(queries), np.uint8)
    seen[queries.index(iSeen)] = 1
    return Case("local", "local_edges", k, d, EDGE_POSE, P, 1.0, slots=slots, queries=queries, query_seen=seen)


def local_scene(name, seed, pose, npts, nextra, th, nq=None):
    """A generic scene: the table, a frame with a keypoint for most points, slots holding some of them (good, bad, without
    observations), the local points in a shuffled order, some of them flagged as seen."""
    rng = np.random.RandomState(seed)
    P = generic_points(rng, pose, npts)
    k, d, owner = keypoints_for(rng, pose, P, [j for j in range(npts) if j % 6 != 1], nextra)
    slots = np.full(len(k), -1, np.int32)
    for i in np.flatnonzero(owner >= 0)[::9]:
        slots[i] = owner[i]
    free = [j for j in range(npts) if j % 6 == 1]                              # points without a keypoint of their own, in other slots
    for i, j in zip(np.flatnonzero(owner < 0)[::3], free[::2]):
        slots[i] = j
    q = rng.permutation(npts)[:npts - 7 if nq is None else nq]
    seen = (rng.randint(0, 25, len(q)) == 0).astype(np.uint8)
    return Case("local", name, k, d, pose, P, th, slots=slots, queries=q, query_seen=seen)


def local_nothing_to_match():
    rng = np.random.RandomState(5)
    P = _finish_points([pt((0, 0, -4)), pt((0, 0, 4), bad=True), pt((9, 0, 4)), pt((0, 0, 4), (0, 0, 0.25))], rng)
    k, d, _ = keypoints_for(rng, EDGE_POSE, P, [], 12)
    return Case("local", "local_nothing_to_match", k, d, EDGE_POSE, P, 1.0, slots=None, queries=[0, 1, 2, 3])


def pair_scene(kind, name, seed, pose, npts, nextra, th, n_other=None, ori=True, orb_dist=100):
    """A generic last-frame / key-frame scene: the other frame's keypoints hold table points (some NULL, outliers / found, bad),
    the current frame has a keypoint near most projections and some keypoints that already hold a point."""
    rng = np.random.RandomState(seed)
    P = generic_points(rng, pose, npts)
    k, d, _ = keypoints_for(rng, pose, P, [j for j in range(npts) if j % 6 != 1], nextra, jitter=2.0)
    n_other = npts + 9 if n_other is None else n_other
    op = np.full(n_other, -1, np.int32)
    op[rng.permutation(n_other)[:min(npts, n_other - n_other // 8)]] = rng.permutation(npts)[:min(npts, n_other - n_other // 8)]
    octs = rng.randint(0, NLEVELS, n_other).astype(np.int32)
    for i in np.flatnonzero(op >= 0)[::2]:                                     # every other one on its point's predicted level
        f = _front(pose, P[op[i]])
        octs[i] = f[3] if f else octs[i]
    ok = keys(rng.uniform(-300, 300, n_other), rng.uniform(-220, 220, n_other), octave=octs, angle=rng.uniform(0, 360, n_other).astype(np.float32))
    flag = (rng.randint(0, 12, n_other) == 0).astype(np.uint8)
    has = (rng.randint(0, 15, len(k)) == 0).astype(np.uint8)
    return Case(kind, name, k, d, pose, P, th, other_keys=ok, other_point=op, flag=flag, has=has, ori=ori, orb_dist=orb_dist)


def pair_edges(kind):
    """The identity-pose edges of the two frame-to-frame forms: the zero and negative depths, the bounds, (last frame) a bad point
    that is matched, an outlier and a NULL; (key frame) the depth range, a point behind the camera that is matched, a found and a
    bad point."""
    rng = np.random.RandomState(13 if kind == "last" else 17)
    P = zero_depth_points() + bounds_points()
    iBehind = len(P) - len(bounds_points()) - 1                               # (0.5, 0.25, -4): u = -32, v = -16
    if kind == "kf":
        P += depth_points()
    iBad, iFlag = len(P), len(P) + 1
    P += [pt((1, 1, 4), bad=True, min_d=2, max_d=8), pt((-1, 1, 4), min_d=2, max_d=8), pt((1, -1, 4), min_d=2, max_d=8)]
    _finish_points(P, rng)
    want = [i for i in range(len(P)) if i != iBehind]
    k, d, _ = keypoints_for(rng, EDGE_POSE, P, want, 15)
    # the point behind the camera projects like its mirror image in front of it
    mirror = dict(P[iBehind], pos=-P[iBehind]["pos"])
    kb, db, _ = keypoints_for(rng, EDGE_POSE, [mirror], [0], 0, jitter=0.5)
    k, d = np.concatenate([k, kb]), np.concatenate([d, db])
    n_other = len(P) + 2
    op = np.concatenate([np.arange(len(P)), [-1, -1]]).astype(np.int32)
    octs = np.array([(_front(EDGE_POSE, p) or (0, 0, 0, 0))[3] for p in P] + [0, 0], np.int32)
    if kind == "last":
        octs[iBehind] = int(kb["octave"][0])
    ok = keys(np.zeros(n_other), np.zeros(n_other), octave=octs, angle=rng.uniform(0, 360, n_other).astype(np.float32))
    flag = np.zeros(n_other, np.uint8)
    flag[iFlag] = 1
    return Case(kind, kind + "_edges", k, d, EDGE_POSE, P, 5.0 if kind == "last" else 4.0, other_keys=ok, other_point=op, flag=flag,
                has=None, ori=False, orb_dist=80)


def single_cases():
    """Every single-frame case: per form the edges and generic scenes (about 300 table points and 400 keypoints in the large one);
    th of 1 and of 5 for the local points."""
    return [local_edges(), local_scene("local_scene", 21, generic_pose(1), 300, 180, 1.0), local_scene("local_th5", 22, axis_pose(), 70, 40, 5.0),
            local_nothing_to_match(),
            pair_edges("last"), pair_scene("last", "last_scene", 31, generic_pose(2), 300, 180, 15.0),
            pair_scene("last", "last_axis_no_ori", 32, axis_pose(), 60, 30, 7.0, ori=False),
            pair_edges("kf"), pair_scene("kf", "kf_scene", 41, generic_pose(3), 300, 180, 10.0),
            pair_scene("kf", "kf_axis_th3", 42, axis_pose(), 60, 30, 3.0, orb_dist=64)]


# ---------------------------------------------------------------- batches: 3 frames, 4 pairs, one table
QCAP = 77                        # not a multiple of 64; one pair uses all of it


class Batch:
    """frames: [(keys, desc)]; pairs: [(frame, other frame or None, Case)] -- every Case shares `points`."""

    def __init__(self, kind, frames, pairs, points, qcap):
        self.kind, self.frames, self.pairs, self.points, self.qcap = kind, frames, pairs, points, qcap


def local_batch():
    rng = np.random.RandomState(51)
    poses = [generic_pose(1), generic_pose(2), axis_pose()]
    P = generic_points(rng, poses[0], 90) + generic_points(rng, poses[2], QCAP)
    fr = [keypoints_for(rng, poses[0], P, range(0, 90, 2), 25), keypoints_for(rng, poses[1], P, range(90), 10),
          keypoints_for(rng, poses[2], P, range(90, 90 + QCAP), 30)]

    def slots(f, step):
        s = np.full(len(fr[f][0]), -1, np.int32)
        own = np.flatnonzero(fr[f][2] >= 0)[::step]
        s[own] = fr[f][2][own]
        return s
    mk = lambda name, f, pose, q, sl, th=3.0: Case("local", name, fr[f][0], fr[f][1], pose, P, th, slots=sl, queries=q,
                                                   query_seen=(np.arange(len(q)) % 11 == 4).astype(np.uint8))
    pairs = [(0, None, mk("b_local_0", 0, poses[0], rng.permutation(90)[:60], slots(0, 5))),
             (0, None, mk("b_local_shared_frame", 0, poses[1], rng.permutation(len(P))[:50], slots(0, 7))),
             (1, None, mk("b_local_no_query", 1, poses[1], [], slots(1, 4))),
             (2, None, mk("b_local_full", 2, poses[2], 90 + rng.permutation(QCAP), slots(2, 6)))]
    return Batch("local", [(k, d) for k, d, _ in fr], pairs, P, QCAP)


def pair_batch(kind):
    """qcap = cap = the largest frame (a pair whose other frame it is uses all of qcap); an empty frame gives nq = 0."""
    rng = np.random.RandomState(61 if kind == "last" else 71)
    pose = [generic_pose(1), generic_pose(3), axis_pose()]
    P = generic_points(rng, pose[0], 100)
    f0 = keypoints_for(rng, pose[0], P, range(0, 100, 2), 20, jitter=2.0)
    big = keypoints_for(rng, pose[1], P, range(100), 60, jitter=2.0)             # the largest frame: cap = qcap = its n
    if len(big[0]) % 64 == 0:
        big = tuple(x[:-1] for x in big)
    frames = [(f0[0], f0[1]), (keys([], []), np.zeros((0, 32), np.uint8)), (big[0], big[1])]
    assert len(big[0]) > len(f0[0]) and len(big[0]) % 64 != 0

    def mk(name, cur, oth, ps, th):
        n_o = len(frames[oth][0])
        op = np.full(n_o, -1, np.int32)
        sel = rng.permutation(n_o)[:n_o - n_o // 7]
        op[sel] = rng.randint(0, len(P), len(sel))
        return Case(kind, name, frames[cur][0], frames[cur][1], ps, P, th, other_keys=frames[oth][0], other_point=op,
                    flag=(rng.randint(0, 10, n_o) == 0).astype(np.uint8), has=(rng.randint(0, 12, len(frames[cur][0])) == 0).astype(np.uint8),
                    ori=True, orb_dist=90)
    pairs = [(0, 2, mk("b_%s_full" % kind, 0, 2, pose[0], 9.0)), (0, 2, mk("b_%s_shared_frame" % kind, 0, 2, pose[1], 9.0)),
             (2, 1, mk("b_%s_no_query" % kind, 2, 1, pose[1], 9.0)), (2, 0, mk("b_%s_back" % kind, 2, 0, pose[1], 9.0))]
    return Batch(kind, frames, pairs, P, len(big[0]))


def batches():
    return [local_batch(), pair_batch("last"), pair_batch("kf")]


# ---------------------------------------------------------------- GPU runners
def run_gpu(c, ext):
    """The single call through the Python wrapper."""
    import pilotguru_amd as pg
    F = ArrayFrame(ext, c.keys, c.desc, BOUNDS)
    pts, pd, bad, obs = table_arrays(c.points)
    T = pg.MapPointTable(pts, pd, bad, np.zeros(len(pts) + 1, np.int32), np.zeros(0, np.uint64))
    m = pg.ORBmatcher(c.nnratio, c.ori)
    if c.kind == "local":
        return m.SearchLocalPoints(F, c.pose, c.slots, T, c.queries, c.query_seen, c.th, 0.5, point_has_obs=obs)
    if c.kind == "last":
        return m.SearchByProjectionLastFramePose(F, c.pose, c.other_keys, c.other_point, T, c.th, c.flag, c.has, point_has_obs=obs)
    return m.SearchByProjectionKeyFramePose(F, c.pose, c.other_keys, c.other_point, T, c.th, c.orb_dist, c.flag, c.has)


def run_existing(c, ext, front):
    """The existing matcher of the form, fed with the reference's front-part arrays."""
    import pilotguru_amd as pg
    F = ArrayFrame(ext, c.keys, c.desc, BOUNDS)
    m = pg.ORBmatcher(c.nnratio, c.ori)
    f = front
    if c.kind == "local":
        mp = pg.MapPoints(f["valid"], f["proj_x"], f["proj_y"], f["level"], f["view_cos"], f["pdesc"], f["pobs"])
        return m.SearchByProjection(F, mp, c.th, f["kp_has_point"])
    if c.kind == "last":
        return m.SearchByProjectionLastFrame(F, f["valid"], f["u"], f["v"], f["last_octave"], f["last_angle"], f["pdesc"], f["pobs"], c.th, c.has)
    return m.SearchByProjectionKeyFrame(F, f["valid"], f["found"], f["u"], f["v"], f["dist3d"], f["min_distance"], f["max_distance"],
                                        f["kf_angle"], f["pdesc"], c.th, c.orb_dist, c.has)


def as_batch(c):
    """A single case as a one-pair batch (qcap = its own query count)."""
    if c.kind == "local":
        return Batch("local", [(c.keys, c.desc)], [(0, None, c)], c.points, max(len(c.queries), 1))
    cap = max(len(c.keys), len(c.other_keys))
    return Batch(c.kind, [(c.keys, c.desc), (c.other_keys, np.zeros((len(c.other_keys), 32), np.uint8))], [(0, 1, c)], c.points, cap)


def run_gpu_batch(b, ext, stream=None, raw=False):
    """One launch of the *_batch_device form; returns the per-pair result dicts (raw: the output tensors' bytes as well)."""
    import torch
    L, h = ext._L, ext._h
    keep = []

    def p(t):
        if t is None:
            return None
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = torch.cuda.current_stream() if stream is None else stream
    s = C.c_void_p(st.cuda_stream)
    nf, npair = len(b.frames), len(b.pairs)
    cap = max([len(k) for k, _ in b.frames] + [1])
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    ds = np.full((nf, cap, 32), 0xFF, np.uint8)
    kp["x"], kp["y"] = np.nan, np.nan
    for f, (k, d) in enumerate(b.frames):
        kp[f, :len(k)] = k
        ds[f, :len(k)] = d
    with torch.cuda.stream(st):
        dk, dd = dev(kp.view(np.uint8).reshape(nf, cap, 28)), dev(ds)
        dn = dev(np.array([len(k) for k, _ in b.frames], np.int32))
        gs = torch.empty((nf, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        gi = torch.full((nf, cap), -7, dtype=torch.int32, device="cuda")
        ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), nf, cap, *BOUNDS, p(gs), p(gi), s))
        pts, pd, bad, obs = table_arrays(b.points)
        dpts, dpd, dbad, dobs = dev(pts.view(np.uint8).reshape(len(pts), 32)), dev(pd), dev(bad), dev(obs)
        pose = dev(np.array([c.pose for _, _, c in b.pairs], KF_POSE_DTYPE).view(np.uint8).reshape(npair, -1))
        pf = dev(np.array([f for f, _, _ in b.pairs], np.int32))
        asg = torch.full((npair, cap), -9, dtype=torch.int32, device="cuda")
        nm = torch.full((npair,), -9, dtype=torch.int32, device="cuda")
        qcap = b.qcap

        def rows(get, dtype, width, fill=0):
            x = np.full((npair, width), fill, dtype)
            for j, (_, _, c) in enumerate(b.pairs):
                a = get(c)
                if a is not None:
                    x[j, :len(a)] = a
            return dev(x)
        out = lambda dtype, width: torch.full((npair, width), 77, dtype=dtype, device="cuda")
        if b.kind == "local":
            slots = rows(lambda c: c.slots, np.int32, cap, -1)
            q = rows(lambda c: c.queries, np.int32, qcap, -1)
            seen = rows(lambda c: c.query_seen, np.uint8, qcap)
            nq = dev(np.array([len(c.queries) for _, _, c in b.pairs], np.int32))
            o = dict(in_view=out(torch.uint8, qcap), proj_x=out(torch.float32, qcap), proj_y=out(torch.float32, qcap),
                     level=out(torch.int32, qcap), view_cos=out(torch.float32, qcap), kp_point_out=out(torch.int32, cap),
                     n_to_match=out(torch.int32, 1))
            c0 = b.pairs[0][2]
            ext._check(L.pgorb_search_local_points_batch_device(
                h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), npair, *BOUNDS, p(pose), p(slots), len(pts), p(dpts), p(dpd), p(dbad),
                p(dobs), qcap, p(nq), p(q), p(seen), 0.5, c0.th, c0.nnratio, p(o["in_view"]), p(o["proj_x"]), p(o["proj_y"]), p(o["level"]),
                p(o["view_cos"]), p(o["kp_point_out"]), p(o["n_to_match"]), p(asg), p(nm), s))
            lens = [len(c.queries) for _, _, c in b.pairs]
        else:
            po = dev(np.array([o_ for _, o_, _ in b.pairs], np.int32))
            op = rows(lambda c: c.other_point, np.int32, cap, -1)
            flag = rows(lambda c: c.flag, np.uint8, cap)
            has = rows(lambda c: c.has, np.uint8, cap)
            c0 = b.pairs[0][2]
            if b.kind == "last":
                o = dict(valid=out(torch.uint8, cap), u=out(torch.float32, cap), v=out(torch.float32, cap))
                ext._check(L.pgorb_search_by_projection_last_frame_batch_device(
                    h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(po), npair, *BOUNDS, p(pose), p(has), p(op), p(flag), len(pts),
                    p(dpts), p(dpd), p(dobs), c0.th, int(c0.ori), p(o["valid"]), p(o["u"]), p(o["v"]), p(asg), p(nm), s))
            else:
                o = dict(u=out(torch.float32, cap), v=out(torch.float32, cap), dist3d=out(torch.float32, cap))
                ext._check(L.pgorb_search_by_projection_keyframe_pose_batch_device(
                    h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pf), p(po), npair, *BOUNDS, p(pose), p(has), p(op), p(flag), len(pts),
                    p(dpts), p(dpd), p(dbad), c0.th, c0.orb_dist, int(c0.ori), p(o["u"]), p(o["v"]), p(o["dist3d"]), p(asg), p(nm), s))
            lens = [len(c.other_keys) for _, _, c in b.pairs]
    st.synchronize()
    res = []
    for j, (f, _, c) in enumerate(b.pairs):
        r = dict(nmatches=int(nm[j]), assigned=asg[j, :len(c.keys)].cpu().numpy())
        for key, t in o.items():
            if key == "kp_point_out":
                r[key] = t[j, :len(c.keys)].cpu().numpy()
            elif key == "n_to_match":
                r[key] = int(t[j, 0])
            else:
                r[key] = t[j, :lens[j]].cpu().numpy()
        res.append(r)
    if raw:
        return res, b"".join(t.cpu().numpy().tobytes() for t in [asg, nm] + list(o.values()))
    return res
