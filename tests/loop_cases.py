"""Constructed cases for loop closing's four matchers (pilotguru_amd/csrc/loop.hip; the Scw pair first, then SearchBySim3 and
SearchByBoW between key frames) and the runners that put them through the
plain reference (tests/loop_reference.py), the single-call ABI and the batched device forms.  A helper module (no tests):
tests/test_loop_matchers.py uses it.

A case is one key frame (keypoints and descriptors constructed, not extracted; its pose record is the decomposed Scw), a table of
map points, the key frame's slots -- vpMatched for SearchByProjection, mvpMapPoints for Fuse -- and a query list in which a point
may appear twice.  The front part (projection, image, depth, angle, scale, window) is the one ORBmatcher::Fuse(pKF, points) has,
so its edge cases are fuse_cases' placed by hand; the cases here add what the two routines decide differently."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_cases as FC  # noqa: E402
import fuse_reference as FR  # noqa: E402
import loop_reference as LR  # noqa: E402
from matcher_cases import SF, at_distance, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE  # noqa: E402

f32 = np.float32
BOUNDS, P0, KID = FC.BOUNDS, FC.P0, FC.KID


class Case:
    """kf: (id, keys, desc, pose, bounds); points: fuse_cases' dicts (observations unused); slots[i] = point index or -1;
    queries: point indices; th: an int (SearchByProjection takes one)."""

    def __init__(self, name, kf, points, slots, queries, th=3):
        self.name, self.kf, self.points, self.th = name, kf, points, int(th)
        self.slots = np.asarray(slots, np.int32)
        self.queries = [int(q) for q in queries]
        assert len(self.slots) == len(kf[1])

    def build(self):
        kid, k, d, P, b = self.kf
        kf = FC.make_kf(kid, k, d, P, b)
        mps = []
        for i, p in enumerate(self.points):
            mp = FR.MapPoint(i, p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"])
            mp.bad = bool(p.get("bad", False))
            mps.append(mp)
        slots = [mps[s] if s >= 0 else None for s in self.slots]
        return kf, mps, slots, [mps[q] for q in self.queries]


def _ids(objs):
    return np.array([-1 if o is None else o.id for o in objs], np.int32)


def run_ref3(c, rules=LR.REFERENCE, hits=None):
    """(nmatches, assigned, matched afterwards) of the sequential SearchByProjection."""
    kf, _, matched, q = c.build()
    n, asg = LR.search_by_projection_sim3(kf, q, matched, c.th, rules, hits)
    return n, np.array(asg, np.int32), _ids(matched)


def run_ref4(c, rules=LR.REFERENCE, hits=None):
    """(nFused, action, replace_point, best_idx, best_dist, slots afterwards) of the sequential Fuse."""
    kf, _, slots, q = c.build()
    kf.slots = slots
    n, out = LR.fuse_sim3(kf, q, float(c.th), rules, hits)
    return (n, np.array([o[0] for o in out], np.int32), _ids([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.int32), _ids(kf.slots))


def run_two_pass3(c):
    kf, _, matched, q = c.build()
    n, asg, out = LR.search_by_projection_two_pass(kf, q, matched, c.th)
    return n, np.array(asg, np.int32), _ids(out)


def run_two_pass4(c):
    kf, _, slots, q = c.build()
    kf.slots = slots
    n, out, after = LR.fuse_two_pass(kf, q, float(c.th))
    return (n, np.array([o[0] for o in out], np.int32), _ids([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.int32), _ids(after))


def same(x, y):
    return int(x[0]) == int(y[0]) and len(x) == len(y) and \
        all(np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)) for a, b in zip(x[1:], y[1:]))


# ---------------------------------------------------------------- cases
def from_fuse_case(c):
    """A fuse_cases.Case as a case here: the same key frame, points and slots, the non-NULL queries."""
    return Case(c.name, c.kf, c.points, c.slots(), [q for q in c.queries if q >= 0], th=int(c.th))


FRONT = ["matches", "bad", "in_kf", "behind", "outside", "u_on_max", "depth_min", "depth_min_past", "depth_max", "depth_max_past",
         "angle", "octave_above", "chi2", "tie", "dist_50", "dist_51", "no_candidate", "reading_dot"]


def _cluster(name, rng, kp_dists, nq, slots=None, queries=None, qdist=0, th=3, bad=(), pos=(0.3, 0.2, 4.0), spread=1.0):
    """nq points at (nearly) one place whose descriptors are `qdist` bits from a base, and keypoints around the projection at
    kp_dists bits from it; slots / queries default to empty / every point once."""
    pos = np.array(pos, np.float32)
    u, v, _ = FC.project(P0, pos)
    base = rand_desc(rng)[0]
    kps = [(float(f32(u + rng.uniform(-spread, spread))), float(f32(v + rng.uniform(-spread, spread))), 0) for _ in kp_dists]
    kf = FC._keyframe(kps, [at_distance(base, int(d), rng) for d in kp_dists])
    pts = []
    for i in range(nq):
        p = FC.point(pos + rng.randn(3).astype(np.float32) * 1e-3, rng, level=0)
        p["desc"] = at_distance(base, int(qdist), rng) if qdist else base.copy()
        p["obs"], p["bad"] = [], i in bad
        pts.append(p)
    return Case(name, kf, pts, [-1] * len(kps) if slots is None else slots, range(nq) if queries is None else queries, th)


def edge_cases(seed=0):
    rng = np.random.RandomState(seed)
    by_name = {c.name: c for c in FC.edge_cases()}
    cs = [from_fuse_case(by_name[n]) for n in FRONT]
    # 3: two queries share a best keypoint -- the second takes its next best (taken_skipped); 4: ADDED, then a replace request
    cs.append(_cluster("two_on_one", rng, [2, 9], 2))
    # ... and a third finds nothing left within TH_LOW
    cs.append(_cluster("three_on_two", rng, [2, 9, 60], 3))
    # a point queried twice: 3 matches it twice (spAlreadyFound is the entry set), 4 requests replacing it by itself
    cs.append(_cluster("repeated", rng, [2, 9, 15], 2, queries=[0, 1, 0, 0]))
    # the best keypoint holds a point on entry: 3 skips it (and the holder, queried, is already found); 4 requests the replace
    cs.append(_cluster("occupied", rng, [2, 9], 3, slots=[2, -1], queries=[0, 2, 1]))
    # ... a bad point: 3 still skips the keypoint; 4 reports KF_POINT_BAD and counts the query
    cs.append(_cluster("occupied_bad", rng, [2, 9], 3, slots=[2, -1], queries=[0, 1], bad=(2,)))
    # no query at all; no keypoint at all
    cs.append(_cluster("no_queries", rng, [2, 9], 1, queries=[]))
    c = _cluster("no_keypoints", rng, [], 2)
    cs.append(c)
    return cs


def collision_case(seed, npoints=20, nkeys=6, nocc=2, nrep=5):
    """Many points projecting onto a few keypoints, some of which hold points on entry (one of them bad), with bad queries and
    repeated queries in a random order."""
    rng = np.random.RandomState(1000 + seed)
    c = _cluster("collisions%d" % seed, rng, [int(rng.randint(0, 30)) for _ in range(nkeys)], npoints, qdist=0, spread=1.5)
    base = c.points[0]["desc"].copy()
    for i, p in enumerate(c.points):
        p["desc"] = at_distance(base, int(rng.randint(0, 25)), rng) if rng.rand() < 0.85 else rand_desc(rng)[0]
        p["bad"] = rng.rand() < 0.1
    slots = np.full(nkeys, -1, np.int32)
    holders = rng.choice(npoints, nocc, replace=False)
    slots[rng.choice(nkeys, nocc, replace=False)] = holders
    c.points[int(holders[0])]["bad"] = True
    q = list(rng.permutation(npoints)) + list(rng.choice(npoints, nrep))
    return Case(c.name, c.kf, c.points, slots, [int(x) for x in rng.permutation(q)])


def dense_window_case(rng, nkp=80):
    """One query (th = 10, radius 10 px at level 0) with `nkp` > 64 keypoints of distance <= 50 in its window, then more queries
    at the same place that take the next best ones."""
    dists = [int(x) for x in rng.permutation(np.arange(nkp) % 45 + 3)]
    return _cluster("dense_window", rng, dists, 6, th=10, spread=8.0)


def chain_case(rng, steps=7):
    """Queries with one descriptor at one place and keypoints at distances 1, 2, ...: query k's best is taken by query k - 1."""
    return _cluster("chain", rng, list(range(1, steps + 2)), steps)


def wide_case(seed, npts):
    """npts points all over the image, most with a keypoint near their projection, some contested by a duplicate point."""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-2.2, 2.2, npts), rng.uniform(-1.6, 1.6, npts), rng.uniform(3.5, 6.0, npts)], 1).astype(np.float32)
    pts, kps, ds = [], [], []
    for j in range(npts):
        src = j if j % 5 else max(j - 1, 0)                                   # every fifth point duplicates its predecessor
        lvl = int(rng.choice([0, 0, 1, 2, 3]))
        p = FC.point(X[src], rng, level=lvl)
        if src != j:
            p["desc"] = at_distance(pts[src]["desc"], 4, rng)
        pts.append(p)
        if src == j and rng.rand() < 0.9:
            u, v, _ = FC.project(P0, X[j])
            for _ in range(int(rng.randint(1, 4))):
                kps.append((float(f32(u + rng.uniform(-2, 2))), float(f32(v + rng.uniform(-2, 2))), max(lvl - int(rng.randint(0, 2)), 0)))
                ds.append(at_distance(p["desc"], int(rng.choice([3, 10, 30, 50, 51, 70])), rng))
    slots = np.full(len(kps), -1, np.int32)
    held = rng.choice(len(kps), len(kps) // 10, replace=False)
    slots[held] = rng.choice(npts, len(held), replace=False)
    return Case("wide%d_%d" % (seed, npts), FC._keyframe(kps, ds), pts, slots, range(npts), th=3)


# ---------------------------------------------------------------- GPU runners
def table(points):
    import pilotguru_amd as pg
    pts, pd, pb, st, ob = FC.table_arrays([dict(p, obs=[]) for p in points])
    return pg.MapPointTable(pts, pd, pb, st, ob)


def run_gpu3(c, ext):
    import pilotguru_amd as pg
    kid, k, d, P, b = c.kf
    return pg.ORBmatcher().SearchByProjectionSim3(FC.MC.KeyFrameArrays(ext, k, d), P, c.slots, table(c.points), c.queries, c.th, bounds=b)


def run_gpu4(c, ext):
    import pilotguru_amd as pg
    kid, k, d, P, b = c.kf
    return pg.ORBmatcher().FuseSim3(FC.MC.KeyFrameArrays(ext, k, d), P, c.slots, table(c.points), c.queries, float(c.th), bounds=b)


SENTINEL = -9
LAST_MS = {}                     # tools/next_tier_bench.py --loop-only: the batched runners' `timer` results, by routine


def run_gpu_batched(cases, ext, which, qcap=None, extra=3, timer=None):
    """Every case as one problem of ONE batched call (all cases share th): frames case by case, cap = largest n + extra with NaN
    keypoints past n, one shared table (each case's points offset), queries poisoned past d_nq.  Returns per case the tuple of
    run_ref3 / run_ref4 plus the output entries past d_nq[p] (SENTINEL when unwritten)."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    B = len(cases)
    cap = max(len(c.kf[1]) for c in cases) + extra
    qcap = max(max(len(c.queries) for c in cases), 1) + 4 if qcap is None else qcap
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"] = np.nan, np.nan
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    n = np.zeros(B, np.int32)
    poses = np.zeros(B, KF_POSE_DTYPE)
    slots = np.full((B, cap), 0x7FFF0000, np.int32)
    allpts, off = [], []
    for c in cases:
        off.append(len(allpts))
        allpts += [dict(p, obs=[]) for p in c.points]
    nq = np.zeros(B, np.int32)
    Q = np.full((B, qcap), 0x7FFF0000, np.int32)
    # problem p runs on frame B - 1 - p, so problem and key-frame indices differ: kf_point rows go by key frame (Fuse), matched_in
    # rows by problem (SearchByProjection), keypoints / poses / grids by key frame, queries and outputs by problem
    kfi = np.arange(B - 1, -1, -1).astype(np.int32)
    for pi, c in enumerate(cases):
        kid, k, d, P, b = c.kf
        f = int(kfi[pi])
        assert b == BOUNDS and c.th == cases[0].th and len(c.queries) <= qcap
        n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d; poses[f] = P
        slots[pi if which == 3 else f, :len(k)] = np.where(c.slots >= 0, c.slots + off[pi], -1)
        nq[pi] = len(c.queries)
        Q[pi, :len(c.queries)] = [q + off[pi] for q in c.queries]
    pts, pd, pb, _, _ = FC.table_arrays(allpts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    new = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")  # noqa: E731
    dk, dn = Tt(kp.view(np.uint8).reshape(B, cap, 28)), Tt(n)
    gs = torch.zeros((B, 3073), dtype=torch.int32, device="cuda")
    gi = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_frame_grid_batch_device(hd, p(dk), p(dn), B, cap, *BOUNDS, p(gs), p(gi), s))
    head = [hd, p(dk), p(Tt(ds)), p(dn), cap, p(gs), p(gi), p(Tt(kfi)), B, p(Tt(poses.view(np.uint8))),
            *BOUNDS, p(Tt(slots)), len(allpts), p(Tt(pts.view(np.uint8))), p(Tt(pd)), p(Tt(pb)), qcap, p(Tt(nq)), p(Tt(Q))]
    cnt = new(B)
    out = []
    if which == 3:
        asg, mo = new(B, cap), new(B, cap)
        call = lambda: ext._check(L.pgorb_search_by_projection_sim3_batch_device(*head, int(cases[0].th), p(asg), p(mo), p(cnt), s))  # noqa: E731
        call()
        if timer:
            LAST_MS[3] = timer(call)
        torch.cuda.synchronize()
        for f, c in enumerate(cases):
            nn = len(c.kf[1])
            m = mo[f, :nn].cpu().numpy()
            out.append((int(cnt[f]), asg[f, :nn].cpu().numpy(), np.where(m >= 0, m - off[f], -1).astype(np.int32),
                        torch.cat([asg[f, nn:], mo[f, nn:]]).cpu().numpy()))
    else:
        act, rep, bi, bd, so = new(B, qcap), new(B, qcap), new(B, qcap), new(B, qcap), new(B, cap)
        call = lambda: ext._check(L.pgorb_fuse_sim3_batch_device(*head, float(cases[0].th), p(act), p(rep), p(bi), p(bd), p(so), p(cnt), s))  # noqa: E731
        call()
        if timer:
            LAST_MS[4] = timer(call)
        torch.cuda.synchronize()
        for f, c in enumerate(cases):
            k, nn = int(nq[f]), len(c.kf[1])
            r, sl = rep[f, :k].cpu().numpy(), so[f, :nn].cpu().numpy()
            out.append((int(cnt[f]), act[f, :k].cpu().numpy(), np.where(r >= 0, r - off[f], -1).astype(np.int32), bi[f, :k].cpu().numpy(),
                        bd[f, :k].cpu().numpy(), np.where(sl >= 0, sl - off[f], -1).astype(np.int32),
                        torch.cat([act[f, k:], rep[f, k:], bi[f, k:], bd[f, k:], so[f, nn:]]).cpu().numpy()))
    return out


# ---------------------------------------------------------------- SearchBySim3
class PairCase:
    """Two key frames (keys, desc, pose), their slots into one point table, the Sim3 record and the two already-matched masks."""

    def __init__(self, name, kf1, kf2, points, slots1, slots2, sim3, already1, already2, th=7.5):
        self.name, self.kf1, self.kf2, self.points, self.sim3, self.th = name, kf1, kf2, points, sim3, th
        self.slots1, self.slots2 = np.asarray(slots1, np.int32), np.asarray(slots2, np.int32)
        self.already1, self.already2 = np.asarray(already1, np.uint8), np.asarray(already2, np.uint8)

    def build(self):
        mps = []
        for i, p in enumerate(self.points):
            mp = FR.MapPoint(i, p["pos"], p["normal"], p["min_d"], p["max_d"], p["desc"])
            mp.bad = bool(p.get("bad", False))
            mps.append(mp)
        out = []
        for kid, (k, d, P), sl in ((1, self.kf1, self.slots1), (2, self.kf2, self.slots2)):
            kf = FC.make_kf(kid, k, d, P, BOUNDS)
            kf.slots = [mps[s] if s >= 0 else None for s in sl]
            out.append(kf)
        return out[0], out[1]


def run_ref2(c, rules=LR.REFERENCE2, hits=None):
    kf1, kf2 = c.build()
    n, m = LR.search_by_sim3(kf1, kf2, c.sim3, list(c.already1), list(c.already2), c.th, rules, hits)
    return n, np.array(m, np.int32)


def pair_case(seed, npts=60, s12=1.0, fx2=500.0, n_extra=0):
    """npts physical points seen by two key frames whose maps differ by a Sim3 of scale s12: every key frame has its own map
    points (positions in its own map's world), keypoints near the projections with descriptors 0-110 bits from the point's, some
    points in one key frame only, bad points, clutter keypoints, already-matched slots."""
    import pilotguru_amd as pg
    rng = np.random.RandomState(5000 + seed)
    f64 = np.float64
    R1, R2 = FC.MC.rot(*(rng.randn(3) * 0.05)), FC.MC.rot(*(rng.randn(3) * 0.05))
    P1 = FC.MC.pose(R1, rng.randn(3) * 0.2, 500.0, 320.0, 240.0)
    P2 = FC.MC.pose(R2, rng.randn(3) * 0.2, fx2, 320.0, 240.0)
    R12 = FC.MC.rot(*(rng.randn(3) * 0.03)).astype(np.float32)
    t12 = (rng.randn(3) * 0.1).astype(np.float32)
    s = f32(s12)
    sR12 = (s * R12).astype(np.float32)                                       # the caller's arithmetic, in float here
    sR21 = (f32(1.0 / f64(s)) * R12.T).astype(np.float32)
    t21 = (-(sR21.astype(f64) @ t12.astype(f64))).astype(np.float32)
    sim3 = pg.sim3_record(sR12, t12, sR21, t21)
    n = npts + n_extra
    Xc2 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.5, 7.0, n)], 1)
    Xc1 = (sR12.astype(f64) @ Xc2.T).T + t12.astype(f64)
    T1, T2 = (np.asarray(P["Tcw"], f64).reshape(3, 4) for P in (P1, P2))
    pts, keys1, keys2, d1, d2, sl1, sl2 = [], [], [], [], [], [], []
    for j in range(n):
        base = rand_desc(rng)[0]
        lvl = int(rng.choice([0, 0, 1, 2]))
        for which, Xc, T, keys_, ds, sl in ((1, Xc1[j], T1, keys1, d1, sl1), (2, Xc2[j], T2, keys2, d2, sl2)):
            if rng.rand() < 0.15:
                continue                                                      # not seen by this key frame
            u, v = 500.0 * Xc[0] / Xc[2] + 320.0, 500.0 * Xc[1] / Xc[2] + 240.0
            if not (8 <= u < 632 and 8 <= v < 472):
                continue
            other = Xc2[j] if which == 1 else Xc1[j]                          # the frame the point will be projected INTO
            mx = f32(np.linalg.norm(other) * float(SF[lvl]) * 0.97 * rng.choice([1.0, 1.0, 1.0, 1.0, 1.0, 0.7, 1.6]))   # (0.97: PredictScale's ceil lands on lvl)
            pos = (T[:, :3].T @ (Xc - T[:, 3])).astype(np.float32)
            pts.append(dict(pos=pos, normal=np.array([0, 0, 1], np.float32), min_d=f32(mx / SF[FC.NLEVELS - 1]), max_d=mx,
                            desc=at_distance(base, int(rng.randint(0, 6)), rng), bad=rng.rand() < 0.05, obs=[]))
            nk = int(rng.choice([1, 1, 2]))
            hd = int(rng.choice([3, 10, 20, 45, 52, 95, 100, 101]))
            for k in range(nk):                                               # the last keypoint holds the point and is mostly the nearest
                holder = k == nk - 1
                keys_.append((float(f32(u + rng.uniform(-2.5, 2.5))), float(f32(v + rng.uniform(-2.5, 2.5))),
                              int(np.clip(lvl - (rng.choice([0, 0, 0, 1, -1]) if holder else rng.choice([0, 1, -1])), 0, FC.NLEVELS - 1))))
                ds.append(at_distance(base, hd if holder or rng.rand() < 0.4 else int(rng.choice([30, 70, 110])), rng))   # (0.4: a tie with the holder)
                sl.append(len(pts) - 1 if holder else -1)
    for Xo in ((0.5, 0.2, -3.0), (9.0, 0.0, 4.0)):                               # KF1 slots whose points land behind / outside KF2
        Xc = sR12.astype(f64) @ np.array(Xo) + t12.astype(f64)
        pts.append(dict(pos=(T1[:, :3].T @ (Xc - T1[:, 3])).astype(np.float32), normal=np.array([0, 0, 1], np.float32), min_d=f32(0.1),
                        max_d=f32(50.0), desc=rand_desc(rng)[0], bad=False, obs=[]))
        keys1.append((float(rng.uniform(20, 600)), float(rng.uniform(20, 440)), 0))
        d1.append(rand_desc(rng)[0])
        sl1.append(len(pts) - 1)
    kfs = []
    for keys_, ds in ((keys1, d1), (keys2, d2)):
        kf = FC._keyframe(keys_, ds)
        kfs.append((kf[1], kf[2]))
    a1 = (rng.rand(len(sl1)) < 0.1).astype(np.uint8)
    a2 = (rng.rand(len(sl2)) < 0.1).astype(np.uint8)
    return PairCase("pair%d_s%g_fx%g" % (seed, s12, fx2), kfs[0] + (P1,), kfs[1] + (P2,), pts, sl1, sl2, sim3, a1, a2)


def pair_cases():
    return [pair_case(0), pair_case(1, s12=1.3), pair_case(2, s12=0.8, fx2=540.0), pair_case(3, fx2=470.0), pair_case(4, npts=5),
            PairCase("empty2", *_empty_pair())]


def _empty_pair():
    c = pair_case(7, npts=8)
    k0 = FC._keyframe([], [])
    return c.kf1, (k0[1], k0[2], c.kf2[2]), c.points, c.slots1, [], c.sim3, c.already1, []


def run_gpu2(c, ext):
    import pilotguru_amd as pg
    K1, K2 = (FC.MC.KeyFrameArrays(ext, k, d) for k, d, _ in (c.kf1, c.kf2))
    return pg.ORBmatcher().SearchBySim3(K1, K2, c.kf1[2], c.kf2[2], c.slots1, c.slots2, table(c.points), c.sim3, c.already1, c.already2,
                                        c.th, bounds=BOUNDS)


def run_gpu2_batched(cases, ext, extra=3, timer=None):
    """Every pair case as one pair of ONE pgorb_search_by_sim3_batch_device call.  Frames are laid out KF2s first in REVERSE case
    order, then KF1s, so pair index and frame indices differ; one shared table.  Returns per case (nFound, match12, entries past n1)."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    B = len(cases)
    cap = max(max(len(c.kf1[0]), len(c.kf2[0])) for c in cases) + extra
    kp = np.zeros((2 * B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"] = np.nan, np.nan
    ds = np.full((2 * B, cap, 32), 0xFF, np.uint8)
    n = np.zeros(2 * B, np.int32)
    poses = np.zeros(2 * B, KF_POSE_DTYPE)
    slots = np.full((2 * B, cap), 0x7FFF0000, np.int32)
    al1, al2 = np.ones((B, cap), np.uint8), np.ones((B, cap), np.uint8)
    sims = np.zeros(B, pg_sim3_dtype())
    f1, f2 = np.zeros(B, np.int32), np.zeros(B, np.int32)
    allpts, off = [], []
    for c in cases:
        off.append(len(allpts))
        allpts += c.points
    for p_, c in enumerate(cases):
        f2[p_], f1[p_] = B - 1 - p_, B + p_
        for f, (k, d, P), sl in ((f1[p_], c.kf1, c.slots1), (f2[p_], c.kf2, c.slots2)):
            n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d; poses[f] = P
            slots[f, :len(k)] = np.where(sl >= 0, sl + off[p_], -1)
        al1[p_, :len(c.already1)] = c.already1
        al2[p_, :len(c.already2)] = c.already2
        sims[p_] = c.sim3
    pts, pd, pb, _, _ = FC.table_arrays(allpts)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    dk, dn = Tt(kp.view(np.uint8).reshape(2 * B, cap, 28)), Tt(n)
    gs = torch.zeros((2 * B, 3073), dtype=torch.int32, device="cuda")
    gi = torch.zeros((2 * B, cap), dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_frame_grid_batch_device(hd, p(dk), p(dn), 2 * B, cap, *BOUNDS, p(gs), p(gi), s))
    m12 = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    nf = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    a_ = [hd, p(dk), p(Tt(ds)), p(dn), cap, p(gs), p(gi), p(Tt(f1)), p(Tt(f2)), B, p(Tt(poses.view(np.uint8))), *BOUNDS, p(Tt(slots)),
          len(allpts), p(Tt(pts.view(np.uint8))), p(Tt(pd)), p(Tt(pb)), p(Tt(sims.view(np.uint8))), p(Tt(al1)), p(Tt(al2)),
          float(cases[0].th), p(m12), p(nf), s]
    call = lambda: ext._check(L.pgorb_search_by_sim3_batch_device(*a_))  # noqa: E731
    call()
    if timer:
        LAST_MS[2] = timer(call)
    torch.cuda.synchronize()
    return [(int(nf[i]), m12[i, :len(c.kf1[0])].cpu().numpy(), m12[i, len(c.kf1[0]):].cpu().numpy()) for i, c in enumerate(cases)]


def pg_sim3_dtype():
    import pilotguru_amd as pg
    return pg.SIM3_DTYPE


# ---------------------------------------------------------------- SearchByBoW(KF, KF)
NNRATIO = 0.75                   # LoopClosing's ORBmatcher(0.75, true) (LoopClosing.cc:238)


def featvec(node):
    """The FeatureVector CSR (nodes, starts, features) of per-feature node ids: features sorted by (node, index)."""
    node = np.asarray(node, np.int64)
    order = np.argsort(node, kind="stable")
    ids, first = np.unique(node[order], return_index=True)
    return ids.astype(np.uint32), np.append(first, len(node)).astype(np.int32), order.astype(np.uint32)


class BowCase:
    def __init__(self, name, desc1, ang1, valid1, node1, desc2, ang2, valid2, node2):
        self.name = name
        self.k1 = (np.asarray(desc1, np.uint8).reshape(-1, 32), np.asarray(ang1, np.float32), np.asarray(valid1, np.uint8), featvec(node1))
        self.k2 = (np.asarray(desc2, np.uint8).reshape(-1, 32), np.asarray(ang2, np.float32), np.asarray(valid2, np.uint8), featvec(node2))


def run_ref1(c, rules=LR.REFERENCE1, hits=None):
    n, m = LR.search_by_bow_keyframes(*c.k1, *c.k2, NNRATIO, True, rules, hits)
    return n, np.array(m, np.int32)


def bow_case(seed, n=120, nodes=8, node_shift=0, name=None):
    """n physical features; KF1 and KF2 each see most of them, in their own order, with descriptors a chosen distance apart,
    duplicates competing for one KF2 keypoint, invalid keypoints on both sides and mostly one rotation."""
    rng = np.random.RandomState(7000 + seed)
    base = rand_desc(rng, n)
    pn = rng.randint(0, nodes, n)
    d1, a1, v1, n1, d2, a2, v2, n2 = [], [], [], [], [], [], [], []
    for j in range(n):
        rot = float(rng.choice([0.0, 0.0, 0.0, 0.0, 12.0, 90.0, 90.0, 200.0, 200.0, 300.0]))
        ang = float(rng.uniform(0, 360))
        if rng.rand() < 0.9:
            for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):                 # duplicates contest one KF2 keypoint
                d1.append(at_distance(base[j], int(rng.choice([0, 2, 5])), rng)); a1.append(ang); v1.append(rng.rand() < 0.85); n1.append(pn[j])
        if rng.rand() < 0.9:
            for k in range(int(rng.choice([1, 1, 2]))):
                d2.append(at_distance(base[j], int(rng.choice([8, 20, 40, 47, 50, 50, 51, 60]) if k == 0 else rng.choice([30, 60, 64])), rng))
                a2.append((ang - rot) % 360.0); v2.append(rng.rand() < 0.85); n2.append(pn[j] + node_shift)
    o1, o2 = rng.permutation(len(d1)), rng.permutation(len(d2))
    pick = lambda x, o: [x[i] for i in o]  # noqa: E731
    return BowCase(name or "bow%d" % seed, pick(d1, o1), pick(a1, o1), pick(v1, o1), pick(n1, o1), pick(d2, o2), pick(a2, o2), pick(v2, o2),
                   pick(n2, o2))


def bow_cases():
    return [bow_case(0), bow_case(1, n=200, nodes=1, name="one_big_node"), bow_case(2, n=60, nodes=5, node_shift=100, name="no_common_node"),
            bow_case(3, n=40, nodes=30), bow_case(4, n=300, nodes=3)]


def run_gpu1(c, ext):
    import pilotguru_amd as pg
    m = pg.ORBmatcher(NNRATIO, True)
    return m.SearchByBoWKeyFrames(ext, c.k1[0], c.k1[1], c.k1[2], c.k1[3], c.k2[0], c.k2[1], c.k2[2], c.k2[3])


def run_gpu1_batched(cases, ext, extra=3, timer=None):
    """Every case as one pair of ONE pgorb_search_by_bow_keyframes_batch_device call; KF2s first in reverse order, then KF1s."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    B = len(cases)
    cap = max(max(len(c.k1[1]), len(c.k2[1])) for c in cases) + extra
    kp = np.zeros((2 * B, cap), KEYPOINT_DTYPE)
    ds = np.full((2 * B, cap, 32), 0xFF, np.uint8)
    n, nfv = np.zeros(2 * B, np.int32), np.zeros(2 * B, np.int32)
    fn, ff = np.zeros((2 * B, cap), np.uint32), np.zeros((2 * B, cap), np.uint32)
    fs = np.zeros((2 * B, cap + 1), np.int32)
    v1, v2 = np.ones((B, cap), np.uint8), np.ones((B, cap), np.uint8)
    f1, f2 = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for p_, c in enumerate(cases):
        f2[p_], f1[p_] = B - 1 - p_, B + p_
        for f, (d, a, v, fv), vm in ((f1[p_], c.k1, v1), (f2[p_], c.k2, v2)):
            m = len(a)
            n[f] = m; kp["angle"][f, :m] = a; ds[f, :m] = d; vm[p_, :m] = v
            nfv[f] = len(fv[0]); fn[f, :len(fv[0])] = fv[0]; fs[f, :len(fv[1])] = fv[1]; ff[f, :m] = fv[2]
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    m12 = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    nm = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a_ = [hd, p(Tt(kp.view(np.uint8).reshape(2 * B, cap, 28))), p(Tt(ds)), p(Tt(n)), cap, p(Tt(fn.view(np.int32))), p(Tt(fs)),
          p(Tt(ff.view(np.int32))), p(Tt(nfv)), p(Tt(f1)), p(Tt(f2)), B, p(Tt(v1)), p(Tt(v2)), NNRATIO, 1, p(m12), p(nm), s]
    call = lambda: ext._check(L.pgorb_search_by_bow_keyframes_batch_device(*a_))  # noqa: E731
    call()
    if timer:
        LAST_MS[1] = timer(call)
    torch.cuda.synchronize()
    return [(int(nm[i]), m12[i, :len(c.k1[1])].cpu().numpy()) for i, c in enumerate(cases)]


# ---------------------------------------------------------------- the chain of ComputeSim3: 1 -> masks -> 2 -> 3
def chain_inputs(seed=11):
    """One pair_case whose keypoints also carry vocabulary nodes and angles, and the pose that projects KF2's map into KF1."""
    c = pair_case(seed, npts=80)
    rng = np.random.RandomState(seed)
    nodes1, nodes2 = rng.randint(0, 6, len(c.slots1)), rng.randint(0, 6, len(c.slots2))
    bad = np.array([bool(p.get("bad", False)) for p in c.points])
    valid = lambda sl: np.array([s >= 0 and not bad[s] for s in sl], np.uint8)  # noqa: E731
    b = BowCase("chain", c.kf1[1], c.kf1[0]["angle"], valid(c.slots1), nodes1, c.kf2[1], c.kf2[0]["angle"], valid(c.slots2), nodes2)
    f64 = np.float64
    T2 = np.asarray(c.kf2[2]["Tcw"], f64).reshape(3, 4)
    sR12, t12 = np.asarray(c.sim3["sR12"], f64).reshape(3, 3), np.asarray(c.sim3["t12"], f64)
    s = np.sqrt(sR12[0] @ sR12[0])
    Rcw, tcw = (sR12 / s) @ T2[:, :3], (sR12 @ T2[:, 3] + t12) / s
    P1 = c.kf1[2]
    Pscw = FC.MC.pose(Rcw, -Rcw.T @ tcw, float(P1["fx"]), float(P1["cx"]), float(P1["cy"]))
    return c, b, Pscw


def run_chain(c, b, Pscw, step1, step2, step3):
    """step1(b) -> (n, m12); step2(pair case with masks) -> (n, match12); step3(Case) -> (n, assigned, matched_out)."""
    _, m12 = step1(b)
    a1 = (np.asarray(m12) >= 0).astype(np.uint8)
    a2 = np.zeros(len(c.slots2), np.uint8)
    a2[np.asarray(m12)[np.asarray(m12) >= 0]] = 1                             # GetIndexInKeyFrame(pKF2) of the matched point
    c2 = PairCase("chain2", c.kf1, c.kf2, c.points, c.slots1, c.slots2, c.sim3, a1, a2, c.th)
    n2, s12 = step2(c2)
    both = np.where(np.asarray(m12) >= 0, m12, s12)
    matched = np.where(both >= 0, c.slots2[np.maximum(both, 0)], -1)          # vpMatches12 as points of KF2
    queries = [int(s) for s in c.slots2 if s >= 0]                            # vpLoopMapPoints: KF2's points
    c3 = Case("chain3", (1,) + tuple(c.kf1) + (BOUNDS,), c.points, matched, queries, th=10)
    c3.kf = (1, c.kf1[0], c.kf1[1], Pscw, BOUNDS)
    return (np.asarray(m12), np.asarray(s12)) + tuple(step3(c3))
