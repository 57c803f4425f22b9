"""Constructed cases for ORBmatcher::Fuse (pilotguru_amd/csrc/fuse.hip) and the runners that put them through the plain
reference (tests/fuse_reference.py), the single-call ABI and the batched device form.  A helper module (no tests):
tests/test_fuse.py uses it.

A case is one key frame, a table of map points (pose fields, descriptor, bad flag, observations by key-frame id), the key
frame's slots and a query list.  Key frames are mapping_cases' (pose(), rot(), project(); matcher_cases' keys and descriptors):
the edge cases place a point and the keypoints around its projection by hand, neighbourhood() builds a current key frame and
its targets over shared 3D points with duplicate map points, as LocalMapping::SearchInNeighbors meets them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_reference as FR  # noqa: E402
import mapping_cases as MC  # noqa: E402
import mapping_reference as MR  # noqa: E402
from matcher_cases import SF, at_distance, keys, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE  # noqa: E402

f32 = np.float32
S2 = MC.S2
INV_S2 = np.array([f32(1.0) / f32(s) for s in S2], np.float32)
NLEVELS = MC.NLEVELS
W, H, FOCAL = 640, 480, 500.0


def log_sf():
    return f32(FR._LOG_F()(SF[1]))


def make_kf(kf_id, k, d, P, bounds):
    return FR.KeyFrame(kf_id, k, d, P, bounds, SF, INV_S2, log_sf(), NLEVELS)


# ---------------------------------------------------------------- a case as plain data, rebuilt into objects for every run
class Case:
    """kf: (id, keys, desc, pose, bounds); others: [(id, n keypoints)] of the other key frames points observe; points: dicts
    (pos, normal, min_d, max_d, desc, bad, obs = [(kf id, keypoint index)]); slots[i] = point index or -1 (the key frame's,
    consistent with the points' obs); queries: point indices or -1."""

    def __init__(self, name, kf, points, queries, others=(), th=3.0):
        self.name, self.kf, self.points, self.queries, self.others, self.th = name, kf, points, list(queries), list(others), th

    def build(self):
        kid, k, d, P, b = self.kf
        kf = make_kf(kid, k, d, P, b)
        kfs = {kid: kf}
        rng = np.random.RandomState(sum(map(ord, self.name)))
        for oid, n in self.others:
            ok = keys(np.full(n, 10.0), np.full(n, 10.0))
            kfs[oid] = make_kf(oid, ok, rand_desc(rng, n), P, b)
        mps = []
        for i, p in enumerate(self.points):
            mp = FR.MapPoint(i, p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"])
            for oid, idx in p["obs"]:
                mp.add_observation(kfs[oid], idx)
                kfs[oid].slots[idx] = mp
            mp.bad = bool(p.get("bad", False))
            mps.append(mp)
        for i, p in enumerate(self.points):                                    # a bad point kept in a slot (no observations)
            for oid, idx in p.get("bad_slots", ()):
                kfs[oid].slots[idx] = mps[i]
        return kf, kfs, mps, [mps[q] if q >= 0 else None for q in self.queries]

    def slots(self):
        kf, _, _, _ = self.build()
        return np.array([-1 if s is None else s.id for s in kf.slots], np.int32)


def run_reference(c, rules=FR.REFERENCE, hits=None):
    """(nFused, action, best_idx, best_dist, slots afterwards) of the sequential reference."""
    kf, _, _, q = c.build()
    tr = []
    nf = FR.fuse(kf, q, c.th, rules, hits, tr)
    a = np.array([t[0] for t in tr], np.int32)
    return nf, a, np.array([t[1] for t in tr], np.int32), np.array([t[2] for t in tr], np.int32), \
        np.array([-1 if s is None else s.id for s in kf.slots], np.int32)


def same(x, y):
    return int(x[0]) == int(y[0]) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(x[1:], y[1:]))


def table_arrays(points):
    """The map-point table of the ABI from point dicts or MapPoint objects (observations by key-frame id, ascending)."""
    n = len(points)
    pts = np.zeros(max(n, 1), MAP_POINT_DTYPE)
    desc = np.zeros((max(n, 1), 32), np.uint8)
    bad = np.zeros(max(n, 1), np.uint8)
    start = np.zeros(n + 1, np.int32)
    obs = []
    for i, p in enumerate(points):
        if isinstance(p, dict):
            pos, nor, mn, mx, d, b, ids = p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"], p.get("bad", False), \
                sorted(o for o, _ in p["obs"])
        else:
            pos, nor, mn, mx, d, b, ids = p.pos, p.normal, p.min_d, p.max_d, p.desc, p.bad, sorted(k.id for k in p.obs)
        pts[i] = (pos, nor, mn, mx)
        desc[i], bad[i] = d, b
        obs += ids
        start[i + 1] = len(obs)
    return pts[:n], desc[:n], bad[:n], start, np.array(obs, np.uint64)


def run_gpu(c, ext):
    import pilotguru_amd as pg
    kid, k, d, P, b = c.kf
    K = MC.KeyFrameArrays(ext, k, d)
    T = pg.MapPointTable(*table_arrays(c.points))
    return pg.ORBmatcher().Fuse(K, P, kid, c.slots(), T, np.array(c.queries, np.int32), c.th, bounds=b)


# ---------------------------------------------------------------- the edge cases
BOUNDS = (0.0, float(W), 0.0, float(H))
KID = 7
P0 = MC.pose(np.eye(3), (0, 0, 0), FOCAL, W / 2.0, H / 2.0)


def project(P, pos, rules=FR.REFERENCE):
    """What match() computes of a point before the candidates: (u, v, dist3D) under `rules`."""
    T = np.asarray(P["Tcw"], np.float32).reshape(3, 4)
    Ow = np.asarray(P["Ow"], np.float32)
    p = np.asarray(pos, np.float32)
    if rules.gemm == "float":
        pc = [f32(np.float64(MR.gemm3(T[r][0], T[r][1], T[r][2], p[0], p[1], p[2])) + np.float64(T[r][3])) for r in range(3)]
    else:
        pc = [f32(MR._sumprod(T[r][:3], p) + np.float64(T[r][3])) for r in range(3)]
    invz = f32(f32(1) / pc[2])
    u = f32(f32(P["fx"] * f32(pc[0] * invz)) + P["cx"])
    v = f32(f32(P["fy"] * f32(pc[1] * invz)) + P["cy"])
    return u, v, f32(MR.normd([f32(p[i] - Ow[i]) for i in range(3)], MR.Rules(norm=rules.norm)))


def level_of(max_d, dist3d):
    return FR.predict_scale(max_d, dist3d, log_sf(), NLEVELS, FR._LOG_F())


def point(pos, rng, level=0, normal=None, min_d=None, max_d=None, obs=(), bad=False, dist3d=None):
    """A point whose PredictScale gives `level` at its own distance (max_d = dist3D * sf[level]), looking straight back."""
    pos = np.asarray(pos, np.float32)
    d3 = dist3d if dist3d is not None else project(P0, pos)[2]
    mx = f32(d3 * SF[level]) if max_d is None else f32(max_d)
    mn = f32(mx / SF[NLEVELS - 1]) if min_d is None else f32(min_d)
    nrm = (pos / np.linalg.norm(pos)).astype(np.float32) if normal is None else np.asarray(normal, np.float32)
    return dict(pos=pos, normal=nrm, min_d=mn, max_d=mx, desc=rand_desc(rng)[0], bad=bad, obs=list(obs))


def _keyframe(kps, descs):
    k = keys([x for x, _, _ in kps], [y for _, y, _ in kps], octave=np.array([o for _, _, o in kps], np.int32))
    return (KID, k, np.array(descs, np.uint8).reshape(-1, 32), P0, BOUNDS)


def _simple(name, rng, pos, offsets_dists, level=None, queries=None, **pkw):
    """One query point at pos and keypoints at its projection + (dx, dy) with (octave, distance to the point's descriptor)."""
    p = point(pos, rng, level=0 if level is None else level, **pkw)
    u, v, d3 = project(P0, p["pos"])
    lvl = level_of(p["max_d"], d3)
    kps, ds = [], []
    for dx, dy, do, dist in offsets_dists:
        kps.append((float(f32(u + dx)), float(f32(v + dy)), lvl + do))
        ds.append(at_distance(p["desc"], dist, rng))
    return Case(name, _keyframe(kps, ds), [p], [0] if queries is None else queries)


def _bound_for(d3, fac):
    """A float b with fac*b == d3 in float (the getters' 0.8f*mfMinDistance / 1.2f*mfMaxDistance)."""
    b0 = f32(d3 / fac)
    for k in range(0, 9):
        for sgn in (1, -1):
            b = b0
            for _ in range(k):
                b = np.nextafter(b, f32(np.inf) if sgn > 0 else f32(-np.inf), dtype=np.float32)
            if f32(fac * b) == d3:
                return b
    raise AssertionError("no float bound for %r" % d3)


def _search(rng, make, differs, tries=20000):
    for _ in range(tries):
        c = make()
        if c is not None and differs(c):
            return c
    raise AssertionError("no input separates the readings")


def edge_cases(seed=0):
    rng = np.random.RandomState(seed)
    cs = []
    # the skips before the descriptor loop
    base = _simple("matches", rng, (0.3, 0.2, 4.0), [(0.4, -0.3, 0, 10)])
    cs.append(base)
    c = _simple("null", rng, (0.3, 0.2, 4.0), [(0.4, -0.3, 0, 10)], queries=[-1, 0, -1])
    cs.append(c)
    c = _simple("bad", rng, (0.3, 0.2, 4.0), [(0.4, -0.3, 0, 10)], bad=True)
    cs.append(c)
    # in the key frame already: it holds slot 1 (a keypoint it would match again)
    c = _simple("in_kf", rng, (0.3, 0.2, 4.0), [(0.4, -0.3, 0, 10), (0.1, 0.1, 0, 5)])
    c.points[0]["obs"] = [(KID, 1)]
    cs.append(c)
    cs.append(_simple("behind", rng, (0.3, 0.2, -4.0), [(0.4, -0.3, 0, 10)]))
    cs.append(_simple("outside", rng, (3.0, 0.2, 4.0), [(0.0, 0.0, 0, 10)]))
    # u == maxX: rejected by the strict bound (the keypoint just inside would match otherwise)
    x = f32(0.64)
    assert project(P0, (x, 0.0, 1.0))[0] == f32(W)
    # (keypoints within 5 px of the right edge are outside the grid: PosInGrid rounds 63.5 up; level 5 gives a radius of 7.5 px)
    c = _simple("u_on_max", rng, (x, 0.1, 1.0), [(-5.5, 0.0, 0, 10)], level=5)
    cs.append(c)
    # dist3D exactly on both ends of the depth range, and just past each
    pos = np.array([0.2, -0.1, 3.0], np.float32)
    d3 = project(P0, pos)[2]
    for tag, fac in (("min", f32(0.8)), ("max", f32(1.2))):
        bound = _bound_for(d3, fac)
        past = bound
        while f32(fac * past) == d3:                                          # min: 0.8*min > dist3D; max: 1.2*max < dist3D
            past = np.nextafter(past, f32(np.inf) if tag == "min" else f32(-np.inf), dtype=np.float32)
        for name, b in (("", bound), ("_past", past)):
            kw = dict(min_d=b) if tag == "min" else dict(max_d=b, min_d=f32(d3 / 4))
            cs.append(_simple("depth_%s%s" % (tag, name), rng, pos, [(0.3, 0.2, 0, 12)], **kw))
    # the 60 degree test: a normal at 80 degrees is rejected
    pos = np.array([0.1, 0.0, 5.0], np.float32)
    n80 = np.array([np.sin(np.radians(80)), 0.0, np.cos(np.radians(80))], np.float32)
    cs.append(_simple("angle", rng, pos, [(0.3, 0.2, 0, 12)], normal=n80))
    # octave level + 1 is not searched (the nearer, closer keypoint), level - 1 is
    cs.append(_simple("octave_above", rng, (0.5, 0.3, 6.0), [(0.2, 0.2, 1, 3), (0.9, -0.5, 0, 20), (-0.6, 0.4, -1, 25)], level=2))
    # chi-square: e2 * invSigma2 just above 5.99 and just below
    e = float(np.sqrt(5.99 / float(INV_S2[0]) / 2.0))
    cs.append(_simple("chi2", rng, (0.2, 0.3, 4.0), [(e * 1.001, e * 1.001, 0, 3), (e * 0.99, e * 0.99, 0, 30)]))
    # distance ties: the first in scan order wins; 50 fuses and 51 does not
    cs.append(_simple("tie", rng, (0.25, -0.2, 4.0), [(0.5, 0.5, 0, 17), (-0.5, -0.5, 0, 17), (0.2, -0.6, 0, 17)]))
    cs.append(_simple("dist_50", rng, (0.25, -0.2, 4.0), [(0.5, 0.5, 0, 50), (-0.5, -0.5, 0, 60)]))
    cs.append(_simple("dist_51", rng, (0.25, -0.2, 4.0), [(0.5, 0.5, 0, 51), (-0.5, -0.5, 0, 52)]))
    cs.append(_simple("no_candidate", rng, (0.25, -0.2, 4.0), [(9.0, 9.0, 0, 1)]))
    cs += chain_cases(rng)
    cs += reading_cases(rng)
    return cs


def chain_cases(rng):
    """Slot chains of length 1-3 over empty, bad and live occupants: equal counts, overlapping observation sets."""
    cs = []
    others = [(100 + i, 16) for i in range(10)]
    used = {}
    pos = np.array([0.3, 0.2, 4.0], np.float32)

    def q(obs_ids, d, bad=False):
        p = point(pos, rng, level=0)
        p["obs"] = []
        for i in obs_ids:                                                    # distinct keypoints of each other key frame
            used[i] = used.get(i, -1) + 1
            p["obs"].append((i, used[i]))
        p["desc"] = d
        p["bad"] = bad
        return p

    def case(name, occ_obs, queries_obs, occ_bad=False):
        base = rand_desc(rng)[0]
        u, v, _ = project(P0, pos)
        kf = _keyframe([(float(f32(u + 0.4)), float(f32(v - 0.3)), 0), (float(f32(u - 3.0)), float(f32(v + 2.0)), 0)],
                       [base, rand_desc(rng)[0]])
        pts = []
        if occ_obs is not None:
            o = q(occ_obs, at_distance(base, 3, rng))
            o["obs"] = [(KID, 0)] + o["obs"]
            if occ_bad:
                o["bad"], o["bad_slots"], o["obs"] = True, [(KID, 0)], []
            pts.append(o)
        for k, ob in enumerate(queries_obs):
            pts.append(q(ob, at_distance(base, 5 + 3 * k, rng)))
        first = 1 if occ_obs is not None else 0
        return Case(name, kf, pts, list(range(first, len(pts))), others=others)
    cs.append(case("chain1_empty", None, [[100, 101]]))
    cs.append(case("chain2_empty", None, [[100, 101], [102, 103, 104]]))
    cs.append(case("chain3_empty", None, [[100], [101, 102], [103]]))
    cs.append(case("chain1_bad", [100], [[101, 102]], occ_bad=True))
    cs.append(case("chain2_bad", [100], [[101], [102, 103]], occ_bad=True))
    cs.append(case("chain1_live_more", [100, 101, 102], [[103, 104]]))
    cs.append(case("chain1_live_tie", [100, 101], [[102, 103, 104]]))               # occupant 3 (kf included) vs query 3
    cs.append(case("chain1_live_less", [100], [[101, 102, 103]]))
    # union != sum: the occupant {K, 100, 101} absorbs {100, 102} (union 4, sum 5), then a query of 4 takes the slot
    cs.append(case("chain2_overlap", [100, 101], [[100, 102], [103, 104, 105, 106]]))
    # a query takes the slot (tie), absorbs the occupant's set, then a later one with overlap merges into it
    cs.append(case("chain3_overlap", [100], [[101], [100, 101, 102], [101, 103, 104]]))
    cs.append(case("chain3_live", [100, 101], [[102], [103, 104, 105], [100, 106, 107, 108, 109]]))
    return cs


def reading_cases(rng):
    """Inputs on which the cv::Mat readings decide: gemm (u just at mnMaxX), norm (dist3D at the range bound), dot (60 deg)."""
    cs = []
    alt = {"gemm": FR.Rules(gemm="double"), "norm": FR.Rules(norm="float"), "dot": FR.Rules(dot="float")}

    def runs_differ(c, rules):
        return not same(run_reference(c), run_reference(c, rules))

    def make_gemm():
        R = MC.rot(*(rng.randn(3) * 0.3))
        P = MC.pose(R, rng.randn(3) * 0.5, FOCAL, W / 2.0, H / 2.0)
        z = rng.uniform(2, 6)
        Xc = np.array([(W - W / 2.0) / FOCAL * z, rng.uniform(-0.3, 0.3) * z, z])
        T = np.asarray(P["Tcw"], np.float64).reshape(3, 4)
        pos = (T[:, :3].T @ (Xc - T[:, 3])).astype(np.float32)
        ua, va, d3 = project(P, pos)
        ub, _, _ = project(P, pos, alt["gemm"])
        if ua == ub or not (min(ua, ub) < W <= max(ua, ub)):
            return None
        p = point(pos, rng, level=5, dist3d=d3, normal=((pos - P["Ow"]) / d3).astype(np.float32))
        kp = keys([634.5], [float(va)], octave=5)
        return Case("reading_gemm", (KID, kp, at_distance(p["desc"], 9, rng).reshape(1, 32), P, BOUNDS), [p], [0])
    cs.append(_search(rng, make_gemm, lambda c: runs_differ(c, alt["gemm"]), 200000))

    def make_norm():
        pos = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 6)], np.float32)
        da, db = project(P0, pos)[2], project(P0, pos, alt["norm"])[2]
        if da == db:
            return None
        mx = f32(min(da, db) / f32(1.2))
        while f32(f32(1.2) * mx) < min(da, db):
            mx = np.nextafter(mx, f32(np.inf), dtype=np.float32)
        while f32(f32(1.2) * mx) > min(da, db):
            mx = np.nextafter(mx, f32(-np.inf), dtype=np.float32)
        p = point(pos, rng, max_d=mx, min_d=f32(mx / 8))
        u, v, _ = project(P0, pos)
        kp = keys([float(f32(u + 0.3))], [float(v)], octave=level_of(mx, da))
        return Case("reading_norm", (KID, kp, at_distance(p["desc"], 9, rng).reshape(1, 32), P0, BOUNDS), [p], [0])
    cs.append(_search(rng, make_norm, lambda c: runs_differ(c, alt["norm"])))

    def make_dot():
        pos = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 6)], np.float32)
        d3 = project(P0, pos)[2]
        a = pos / np.linalg.norm(pos)
        perp = np.cross(a, rng.randn(3))
        perp /= np.linalg.norm(perp)
        t = np.radians(60.0) + rng.randn() * 1e-8
        n = (a * np.cos(t) + perp * np.sin(t)).astype(np.float32)
        ra = MR.dotd(list(pos), list(n)) < 0.5 * np.float64(d3)
        rb = MR.dotd(list(pos), list(n), MR.Rules(norm="float")) < 0.5 * np.float64(d3)
        if ra == rb:
            return None
        p = point(pos, rng, level=0, normal=n, dist3d=d3)
        u, v, _ = project(P0, pos)
        kp = keys([float(f32(u + 0.3))], [float(v)], octave=0)
        return Case("reading_dot", (KID, kp, at_distance(p["desc"], 9, rng).reshape(1, 32), P0, BOUNDS), [p], [0])
    cs.append(_search(rng, make_dot, lambda c: runs_differ(c, alt["dot"]), 400000))
    return cs


# ---------------------------------------------------------------- SearchInNeighbors scenes
def neighbourhood(seed, w=640, h=480, ntargets=20, npts=1000, focal=500.0):
    """A current key frame (id 1000) and `ntargets` targets (ids 1001..) over npts 3D points.  Every physical point may have an
    'old' map point observed by some targets and a 'new' one observed by the current key frame (and one target): the duplicates
    SearchInNeighbors fuses.  Some slots hold bad points.  Returns (current, targets, points) as fuse_reference objects."""
    rng = np.random.RandomState(seed)
    cx, cy = w / 2.0, h / 2.0
    poses = [MC.pose(np.eye(3), (0, 0, 0), focal, cx, cy)]
    for t in range(ntargets):
        if t % 7 == 6:
            R, C = np.eye(3), (0.0, 0.0, 5.0)                              # far ahead: many points behind it
        else:
            R, C = MC.rot(rng.randn() * 0.02, rng.randn() * 0.08, rng.randn() * 0.02), rng.randn(3) * np.array([0.4, 0.2, 0.3])
        poses.append(MC.pose(R, C, focal, cx, cy))
    X = np.stack([rng.uniform(-4, 4, npts), rng.uniform(-3, 3, npts), rng.uniform(2.5, 10, npts)], 1)
    D = rand_desc(rng, npts)
    lvl = rng.choice([0, 0, 0, 1, 1, 2, 3, 5], npts)
    bounds = (0.0, float(w), 0.0, float(h))
    kfs, where = [], []
    for k, P in enumerate(poses):
        ks, ds, js = [], [], []
        for j in range(npts):
            u, v, z = MC.project(P, X[j])
            if z <= 0 or not (0 <= u < w and 0 <= v < h) or rng.rand() > 0.75:
                continue
            err = rng.choice([0.0, 0.3, 0.8, 1.5, 3.0]) * SF[lvl[j]]
            a = rng.uniform(0, 2 * np.pi)
            o = int(np.clip(lvl[j] + rng.choice([0, 0, 0, -1, 1]), 0, NLEVELS - 1))
            ks.append((u + err * np.cos(a), v + err * np.sin(a), o))
            ds.append(at_distance(D[j], int(rng.choice([2, 6, 12, 25, 40, 48, 55, 70])), rng))
            js.append(j)
        for _ in range(len(ks) // 10):                                       # clutter
            ks.append((rng.uniform(0, w), rng.uniform(0, h), int(rng.randint(0, 4))))
            ds.append(rand_desc(rng)[0])
            js.append(-1)
        order = rng.permutation(len(ks))
        kk = keys([ks[i][0] for i in order], [ks[i][1] for i in order], octave=np.array([ks[i][2] for i in order], np.int32))
        kfs.append(make_kf(1000 + k, kk, np.array([ds[i] for i in order], np.uint8), P, bounds))
        where.append({js[i]: r for r, i in enumerate(order) if js[i] >= 0})
    points = []

    def new_point(j, observers):
        ref = observers[0]
        Ow = np.asarray(kfs[ref].pose["Ow"], np.float64)
        dist = float(np.linalg.norm(X[j] - Ow))
        nrm = np.mean([(X[j] - np.asarray(kfs[k].pose["Ow"], np.float64)) / np.linalg.norm(X[j] - np.asarray(kfs[k].pose["Ow"], np.float64))
                       for k in observers], 0)
        mx = f32(dist * float(SF[lvl[j]]))
        mp = FR.MapPoint(len(points), X[j].astype(np.float32), nrm.astype(np.float32), f32(mx / SF[NLEVELS - 1]), mx,
                         at_distance(D[j], int(rng.randint(0, 8)), rng))
        for k in observers:
            mp.add_observation(kfs[k], where[k][j])
            kfs[k].slots[where[k][j]] = mp
        points.append(mp)
        return mp
    for j in range(npts):
        seen = [k for k in range(1, len(kfs)) if j in where[k]]
        old = [k for k in seen if rng.rand() < 0.5][:4]
        if old and rng.rand() < 0.8:
            new_point(j, old)
        if j in where[0]:
            if rng.rand() < 0.6:
                extra = [k for k in seen if k not in old][:1] if rng.rand() < 0.3 else []
                new_point(j, [0] + extra)
    for k in range(len(kfs)):                                               # a few bad points left in slots
        free = [i for i in range(len(kfs[k].keys)) if kfs[k].slots[i] is None]
        for i in rng.choice(free, min(len(free), 3), replace=False) if free else []:
            mp = FR.MapPoint(len(points), (0, 0, 1), (0, 0, 1), 1, 2, rand_desc(rng)[0])
            mp.bad = True
            kfs[k].slots[int(i)] = mp
            points.append(mp)
    return kfs[0], kfs[1:], points


def map_state(kfs, points):
    """Everything Fuse changes: every key frame's slots, every point's bad flag, observation set and descriptor."""
    return ([[-1 if s is None else s.id for s in kf.slots] for kf in kfs],
            [(p.bad, sorted((k.id, i) for k, i in p.obs.items()), p.desc.tobytes()) for p in points])


def apply_actions(kf, queries, action, best_idx):
    """Replays pgorb_fuse's actions in query order against the host map (include/pgorb.h): Replace, AddObservation + AddMapPoint."""
    for mp, a, bi in zip(queries, action, best_idx):
        a, bi = int(a), int(bi)
        if a == FR.ADDED:
            mp.add_observation(kf, bi)
            kf.slots[bi] = mp
        elif a == FR.MERGED:
            mp.replace(kf.slots[bi])
        elif a == FR.REPLACED:
            kf.slots[bi].replace(mp)


def gpu_fuse_objects(ext, kf, queries, points, th=3.0):
    """One pgorb_fuse of fuse_reference objects through the Python mirror."""
    import pilotguru_amd as pg
    T = pg.MapPointTable(*table_arrays(points))
    K = MC.KeyFrameArrays(ext, kf.keys, kf.desc)
    slots = np.array([-1 if s is None else s.id for s in kf.slots], np.int32)
    q = np.array([-1 if p is None else p.id for p in queries], np.int32)
    return pg.ORBmatcher().Fuse(K, kf.pose, kf.id, slots, T, q, th, bounds=kf.bounds)


def search_in_neighbors_gpu(ext, current, targets, points, th=3.0, seen_actions=None):
    """SearchInNeighbors with one pgorb_fuse per target in order, the actions applied on the host between calls, then the fuse of
    the targets' points into the current key frame."""
    vp = list(current.slots)
    res = []
    for kf in targets:
        nf, a, bi, _, _ = gpu_fuse_objects(ext, kf, vp, points, th)
        apply_actions(kf, vp, a, bi)
        res.append(nf)
        if seen_actions is not None:
            seen_actions.update(int(x) for x in a)
    cand, seen = [], set()
    for kf in targets:
        for mp in list(kf.slots):
            if mp is None or mp.bad or mp.id in seen:
                continue
            seen.add(mp.id)
            cand.append(mp)
    nf, a, bi, _, _ = gpu_fuse_objects(ext, current, cand, points, th)
    apply_actions(current, cand, a, bi)
    if seen_actions is not None:
        seen_actions.update(int(x) for x in a)
    res.append(nf)
    return res


def run_gpu_batched(cases, ext, extra=3, qextra=4):
    """Every case as one problem of ONE pgorb_fuse_batch_device call: frames case by case, cap = largest n + extra with NaN
    keypoints past n, one shared table (each case's points offset), queries padded with poison past d_nq.  Returns per case
    (nFused, action, best_idx, best_dist, slots)."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    B = len(cases)
    cap = max(len(c.kf[1]) for c in cases) + extra
    qcap = max(max(len(c.queries) for c in cases), 1) + qextra
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"] = np.nan, np.nan
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    n = np.zeros(B, np.int32)
    ids = np.zeros(B, np.uint64)
    poses = np.zeros(B, KF_POSE_DTYPE)
    slots = np.full((B, cap), 0x7FFF0000, np.int32)
    allpts, off = [], []
    for f, c in enumerate(cases):
        off.append(len(allpts))
        allpts += c.points
    nq = np.zeros(B, np.int32)
    Q = np.full((B, qcap), 0x7FFF0000, np.int32)                            # poison past nq
    for f, c in enumerate(cases):
        kid, k, d, P, b = c.kf
        assert b == BOUNDS
        n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d; ids[f] = kid; poses[f] = P
        sl = c.slots()
        slots[f, :len(k)] = np.where(sl >= 0, sl + off[f], -1)
        nq[f] = len(c.queries)
        Q[f, :len(c.queries)] = [q + off[f] if q >= 0 else -1 for q in c.queries]
    pts, pd, pb, st, ob = table_arrays(allpts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dk = Tt(kp.view(np.uint8).reshape(B, cap, 28))
    dn = Tt(n)
    gs = torch.zeros((B, 3073), dtype=torch.int32, device="cuda")
    gi = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_frame_grid_batch_device(hd, p(dk), p(dn), B, cap, *BOUNDS, p(gs), p(gi), s))
    act = torch.full((B, qcap), -9, dtype=torch.int32, device="cuda")
    bi = torch.full((B, qcap), -9, dtype=torch.int32, device="cuda")
    bd = torch.full((B, qcap), -9, dtype=torch.int32, device="cuda")
    so = torch.full((B, cap), -9, dtype=torch.int32, device="cuda")
    nf = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    ob_t = Tt(ob.view(np.int64)) if len(ob) else torch.zeros(1, dtype=torch.int64, device="cuda")
    ext._check(L.pgorb_fuse_batch_device(hd, p(dk), p(Tt(ds)), p(dn), cap, p(gs), p(gi), p(Tt(np.arange(B, dtype=np.int32))), B,
                                         p(Tt(ids.view(np.int64))), p(Tt(poses.view(np.uint8))), *BOUNDS, p(Tt(slots)), len(allpts),
                                         p(Tt(pts.view(np.uint8))), p(Tt(pd)), p(Tt(pb)), p(Tt(st)), p(ob_t), qcap, p(Tt(nq)), p(Tt(Q)),
                                         float(cases[0].th), p(act), p(bi), p(bd), p(so), p(nf), s))
    torch.cuda.synchronize()
    out = []
    for f, c in enumerate(cases):
        k = int(nq[f])
        sl = so[f, :n[f]].cpu().numpy()
        out.append((int(nf[f]), act[f, :k].cpu().numpy(), bi[f, :k].cpu().numpy(), bd[f, :k].cpu().numpy(),
                    np.where(sl >= 0, sl - off[f], -1).astype(np.int32), act[f, k:].cpu().numpy()))
    return out


def collision_case(seed, npoints=20, nkeys=6, nocc=3, nnull=4):
    """Many points projecting onto a few keypoints: long slot chains over empty, bad and live occupants, with overlapping
    observation sets (ids 100..105), bad queries and NULL entries, in a random order."""
    rng = np.random.RandomState(seed)
    pos = np.array([0.3, 0.2, 4.0], np.float32)
    u, v, _ = project(P0, pos)
    base = rand_desc(rng)[0]
    kps = [(float(f32(u + rng.uniform(-1.5, 1.5))), float(f32(v + rng.uniform(-1.5, 1.5))), 0) for _ in range(nkeys)]
    kf = _keyframe(kps, [at_distance(base, int(rng.randint(0, 40)), rng) for _ in range(nkeys)])
    others = [(100 + i, npoints + 1) for i in range(6)]
    pts = []
    for i in range(npoints):
        p = point(pos + rng.randn(3).astype(np.float32) * 1e-3, rng, level=0)
        p["desc"] = at_distance(base, int(rng.randint(0, 30)), rng) if rng.rand() < 0.85 else rand_desc(rng)[0]
        ids = sorted(rng.choice(6, int(rng.randint(0, 5)), replace=False))
        p["obs"] = [(100 + int(k), i) for k in ids]
        p["bad"] = rng.rand() < 0.1
        if p["bad"]:
            p["obs"] = []
        pts.append(p)
    for slot, i in zip(rng.choice(nkeys, nocc, replace=False), rng.choice(npoints, nocc, replace=False)):
        if pts[i]["bad"]:
            pts[i]["bad_slots"] = [(KID, int(slot))]
        else:
            pts[i]["obs"] = [(KID, int(slot))] + pts[i]["obs"]
    q = list(rng.permutation(npoints)) + [-1] * nnull
    q = [int(x) for x in rng.permutation(q)]
    return Case("collisions%d" % seed, kf, pts, q, others=others)
