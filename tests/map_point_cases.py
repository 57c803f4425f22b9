"""Constructed cases for the map-point refresh (pilotguru_amd/csrc/map_point.hip) and the runners that put them through the plain
reference (tests/map_point_reference.py), the single-call ABI and the batched device form.  A helper module (no tests):
tests/test_map_point_refresh.py uses it.

A case is a list of key frames (keypoints, descriptors, pose, bad flag), a table of map points (position, descriptor, pose fields,
bad flag, an ordered observation list of (key frame, keypoint) and the list position of the reference key frame), a selection
(None = every point) and `what`.  Key frames are mapping_cases' (pose(), rot()); keys and descriptors are matcher_cases'."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_point_reference as MPR  # noqa: E402
import mapping_cases as MC  # noqa: E402
from matcher_cases import SF, at_distance, keys, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE  # noqa: E402

f32 = np.float32
NLEVELS = MC.NLEVELS
MAX_OBS = MPR.MAX_OBS


class Case:
    """kfs: [(keys, desc, pose, bad)]; points: dicts (pos, desc, normal, min_d, max_d, bad, obs = [(kf, keypoint)], ref)."""

    def __init__(self, name, kfs, points, select=None, what=MPR.BOTH):
        self.name, self.kfs, self.points, self.select, self.what = name, kfs, points, select, what

    def build(self):
        K = [MPR.KeyFrame(k, d, P["Ow"], bad) for k, d, P, bad in self.kfs]
        pts = []
        for p in self.points:
            mp = MPR.MapPoint(p["pos"], p["desc"], p["normal"], p["min_d"], p["max_d"], p["bad"])
            mp.obs = [(K[f], i) for f, i in p["obs"]]
            mp.ref = K[p["obs"][p["ref"]][0]] if p["obs"] else None
            pts.append(mp)
        return K, pts

    def selection(self):
        return list(range(len(self.points))) if self.select is None else list(self.select)


def table_arrays(points):
    """The table of the ABI: (points, descriptors, bad, obs_start, obs_frame, obs_idx, ref_obs)."""
    n = len(points)
    pts = np.zeros(n, MAP_POINT_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    bad = np.zeros(n, np.uint8)
    start = np.zeros(n + 1, np.int32)
    of, oi = [], []
    ref = np.zeros(n, np.int32)
    for i, p in enumerate(points):
        pts[i] = (p["pos"], p["normal"], p["min_d"], p["max_d"])
        desc[i], bad[i], ref[i] = p["desc"], p["bad"], p["ref"]
        of += [f for f, _ in p["obs"]]
        oi += [k for _, k in p["obs"]]
        start[i + 1] = len(of)
    return pts, desc, bad, start, np.array(of, np.int32), np.array(oi, np.int32), ref


def run_reference(c, rules=MPR.REFERENCE, hits=None, what=None):
    """(points, descriptors, best_obs, status) as the library reports them: the table afterwards and one entry per selected point."""
    _, pts = c.build()
    what = c.what if what is None else what
    sel = c.selection()
    if hits is not None:
        hits["what_%d" % what] += 1
        if len(sel) < len(pts):
            hits["selection_skips"] += 1
        used = [set(f for f, _ in p["obs"]) for p in c.points]
        if any(used[a] & used[b] for a in range(len(used)) for b in range(a)):
            hits["shared_kfs"] += 1
    best, status = [], []
    for i in sel:
        s, b = MPR.refresh(pts[i], SF, NLEVELS, what, rules, hits)
        status.append(s)
        best.append(b)
    out = np.zeros(len(pts), MAP_POINT_DTYPE)
    for i, mp in enumerate(pts):
        out[i] = (mp.pos, mp.normal, mp.min_d, mp.max_d)
    return out, np.array([mp.desc for mp in pts], np.uint8).reshape(-1, 32), np.array(best, np.int32), np.array(status, np.int32)


def same(x, y):
    """Two results equal: the floats as bit patterns, everything else as integers."""
    return all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() and np.shape(a) == np.shape(b) for a, b in zip(x, y))


def run_gpu(c, ext, what=None):
    import pilotguru_amd as pg
    K = [MC.KeyFrameArrays(ext, k, d) for k, d, _, _ in c.kfs]
    pts, desc, bad, st, of, oi, ref = table_arrays(c.points)
    return pg.LocalMapping.RefreshMapPoints(K, [P for _, _, P, _ in c.kfs], pts, desc, st, of, oi, ref, bad, [b for _, _, _, b in c.kfs],
                                            None if c.select is None else np.array(c.select, np.int32), c.what if what is None else what,
                                            ext=ext)


# ---------------------------------------------------------------- building blocks
def make_kfs(rng, nkf, nkeys=6, bad=()):
    """nkf key frames around the origin looking down +z, nkeys keypoints each with random descriptors and octaves."""
    out = []
    for f in range(nkf):
        R = MC.rot(*(rng.randn(3) * 0.05))
        P = MC.pose(R, rng.randn(3) * np.array([0.8, 0.4, 0.3]), 500.0, 320.0, 240.0)
        k = keys(rng.uniform(20, 620, nkeys), rng.uniform(20, 460, nkeys), octave=rng.randint(0, NLEVELS, nkeys).astype(np.int32))
        out.append((k, rand_desc(rng, nkeys), P, f in bad))
    return out


def make_point(rng, obs, ref=0, bad=False, pos=None):
    pos = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(3, 9)], np.float32) if pos is None else np.asarray(pos, np.float32)
    return dict(pos=pos, desc=rand_desc(rng)[0], normal=rng.randn(3).astype(np.float32), min_d=f32(rng.uniform(0.5, 1)),
                max_d=f32(rng.uniform(5, 9)), bad=bad, obs=list(obs), ref=ref)


def set_descs(kfs, obs, descs):
    """The descriptors of the observed keypoints, in list order."""
    for (f, i), d in zip(obs, descs):
        kfs[f][1][i] = d


def around(rng, n, spread):
    """n descriptors at random distances up to `spread` bits from a common base."""
    base = rand_desc(rng)[0]
    return [at_distance(base, int(rng.randint(0, spread + 1)), rng) for _ in range(n)]


def _one(name, rng, n, nkf=None, ref=0, spread=40, bad_kfs=(), **kw):
    """One point observed by the first n of nkf key frames (keypoint f % nkeys of key frame f)."""
    kfs = make_kfs(rng, nkf or max(n, 1), bad=bad_kfs)
    obs = [(f, int(rng.randint(0, 6))) for f in range(n)]
    set_descs(kfs, obs, around(rng, n, spread))
    return Case(name, kfs, [make_point(rng, obs, ref, **kw)])


def _search(make, differs, tries=4000):
    for _ in range(tries):
        c = make()
        if differs(c):
            return c
    raise AssertionError("no input separates the readings")


def _differs(rules):
    return lambda c: not same(run_reference(c), run_reference(c, rules))


def _medians(c):
    ds = [int.from_bytes(c.kfs[f][1][i].tobytes(), "little") for f, i in c.points[0]["obs"]]
    k = int(0.5 * (len(ds) - 1))
    return [sorted(MPR._dist(a, b) for b in ds)[k] for a in ds]


def edge_cases(seed=0):
    rng = np.random.RandomState(seed)
    M = MPR.MUTANTS
    cs = [_one("empty", rng, 0, nkf=2), _one("bad_point", rng, 3, bad=True), _one("n1", rng, 1), _one("n2", rng, 2)]
    cs.append(_search(lambda: _one("n3", rng, 3), lambda c: run_reference(c)[2][0] != 0))
    # N = 4: the median is sorted_row[1]; a scene on which sorted_row[2] picks another row
    cs.append(_search(lambda: _one("n4_median_index_1", rng, 4), _differs(M["median=n//2"])))
    # equal smallest medians: the first of them wins
    cs.append(_search(lambda: _one("equal_medians", rng, 5, spread=6),
                      lambda c: (lambda m: m.count(min(m)) > 1 and m.index(min(m)) > 0)(_medians(c))))
    cs.append(_search(lambda: _one("best_last", rng, 5), lambda c: (lambda m: m.count(min(m)) == 1 and m[-1] == min(m))(_medians(c))))
    c = _one("identical", rng, 4)
    set_descs(c.kfs, c.points[0]["obs"], [c.kfs[0][1][c.points[0]["obs"][0][1]]] * 4)
    cs.append(c)
    c = _one("dist_256", rng, 3)
    d0 = c.kfs[0][1][c.points[0]["obs"][0][1]]
    set_descs(c.kfs, c.points[0]["obs"], [d0, d0 ^ np.uint8(0xFF), at_distance(d0, 100, rng)])
    cs.append(c)
    # one bad key frame: out of the descriptors (it would have won), in the normal
    cs.append(_search(lambda: _one("one_bad_kf", rng, 4, bad_kfs=(1,)), _differs(M["desc_bad_kf=keep"])))
    cs.append(_one("all_kf_bad", rng, 3, bad_kfs=(0, 1, 2)))
    cs.append(_one("ref_not_first", rng, 5, ref=3))
    c = _one("octave_top", rng, 3, ref=1)
    c.kfs[1][0]["octave"][c.points[0]["obs"][1][1]] = NLEVELS - 1
    cs.append(c)
    c = _one("octave_0", rng, 3, ref=2)
    c.kfs[2][0]["octave"][c.points[0]["obs"][2][1]] = 0
    cs.append(c)
    for n in (63, 64, 65):
        cs.append(_one("n%d" % n, rng, n, ref=n // 2, spread=60))
    cs.append(_one("n_max", rng, MAX_OBS, ref=7, spread=60))
    cs.append(_one("n_max_plus_1", rng, MAX_OBS + 1, ref=7))
    cs.append(_one("n_max_plus_1_bad_point", rng, MAX_OBS + 1, bad=True))
    # several points over shared key frames, every list length from 1 to 40, some bad key frames; a selection that skips points
    kfs = make_kfs(rng, 40, nkeys=48, bad=(5, 17))
    pts = []
    for n in range(1, 41):
        fs = sorted(rng.choice(40, n, replace=False))
        obs = [(int(f), n) for f in fs]
        set_descs(kfs, obs, around(rng, n, 30))
        pts.append(make_point(rng, obs, ref=int(rng.randint(0, n)), bad=(n == 9)))
    cs.append(Case("shared_key_frames", kfs, pts))
    cs.append(Case("selection_skips", kfs, pts, select=[31, 2, 7, 8, 20, 39, 0]))
    cs.append(Case("what_descriptor", kfs, pts, what=MPR.DESCRIPTOR))
    cs.append(Case("what_normal_depth", kfs, pts, what=MPR.NORMAL_DEPTH))
    return cs


# ---------------------------------------------------------------- random scenes
def list_length(rng, nkf):
    """The stated distribution of list lengths: 60 % 1-4 (mostly 2: fresh from CreateNewMapPoints), 25 % 5-12, 10 % 13-40, 4 %
    41-120, 1 % 200-260, clipped to the number of key frames."""
    u = rng.rand()
    if u < 0.60:
        n = int(rng.choice([1, 2, 2, 2, 3, 4]))
    elif u < 0.85:
        n = int(rng.randint(5, 13))
    elif u < 0.95:
        n = int(rng.randint(13, 41))
    elif u < 0.99:
        n = int(rng.randint(41, 121))
    else:
        n = int(rng.randint(200, 261))
    return min(n, nkf)


def random_scene(seed, nkf=22, nkeys=2000, npts=5000, bad_kf_share=0.05, bad_point_share=0.03):
    rng = np.random.RandomState(seed)
    kfs = []
    for f in range(nkf):
        P = MC.pose(MC.rot(*(rng.randn(3) * 0.05)), rng.randn(3) * np.array([1.5, 0.5, 0.5]), 1000.0, 960.0, 540.0)
        k = np.zeros(nkeys, KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(0, 1920, nkeys), rng.uniform(0, 1080, nkeys)
        k["octave"] = rng.choice(NLEVELS, nkeys, p=[.3, .2, .15, .1, .1, .05, .05, .05])
        kfs.append((k, rand_desc(rng, nkeys), P, bool(rng.rand() < bad_kf_share)))
    pts = []
    for _ in range(npts):
        n = list_length(rng, nkf)
        fs = sorted(rng.choice(nkf, n, replace=False))
        obs = [(int(f), int(rng.randint(0, nkeys))) for f in fs]
        set_descs(kfs, obs, around(rng, n, int(rng.choice([4, 20, 60]))))
        pts.append(make_point(rng, obs, ref=int(rng.randint(0, n)), bad=bool(rng.rand() < bad_point_share)))
    return Case("random%d" % seed, kfs, pts)


# ---------------------------------------------------------------- the batched device form
def run_gpu_batched(cases, ext, what, extra_frames=1, extra_keys=3, extra_points=2, extra_out=4):
    """Every case in ONE pgorb_refresh_map_points_batch_device call: frames case by case (cap = largest n + extra_keys, poison past
    n), one table (each case's frame and point indices offset) with extra_points unselected points at its end, the selection the
    concatenation of the cases' selections, outputs extra_out entries longer than nsel and filled with a canary.  Returns per case
    (points, descriptors, best_obs, status) and the check that nothing else was written."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    frames, foff, poff, allpts, sel, cut = [], [], [], [], [], [0]
    for c in cases:
        foff.append(len(frames)); poff.append(len(allpts))
        frames += c.kfs
        for p in c.points:
            q = dict(p)
            q["obs"] = [(f + foff[-1], i) for f, i in p["obs"]]
            allpts.append(q)
        sel += [i + poff[-1] for i in c.selection()]
        cut.append(len(sel))
    rng = np.random.RandomState(1)
    allpts += [make_point(rng, [(0, 0)]) for _ in range(extra_points)]
    B = len(frames) + extra_frames
    cap = max(len(k) for k, _, _, _ in frames) + extra_keys
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["octave"] = np.nan, np.nan, 0x7FFF0000
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    n = np.zeros(B, np.int32)
    poses = np.zeros(B, KF_POSE_DTYPE)
    kb = np.zeros(B, np.uint8)
    for f, (k, d, P, bad) in enumerate(frames):
        n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d; poses[f] = P; kb[f] = bad
    pts, pd, pb, st, of, oi, ref = table_arrays(allpts)
    sel = np.array(sel, np.int32)
    nsel = len(sel)
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_pts, d_pd = Tt(pts.view(np.uint8)), Tt(pd)
    best = torch.full((nsel + extra_out,), -9, dtype=torch.int32, device="cuda")
    status = torch.full((nsel + extra_out,), -9, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_refresh_map_points_batch_device(hd, p(Tt(kp.view(np.uint8).reshape(B, cap, 28))), p(Tt(ds)), p(Tt(n)), B, cap,
                                                       p(Tt(poses.view(np.uint8))), p(Tt(kb)), len(allpts), p(d_pts), p(d_pd), p(Tt(pb)), p(Tt(st)),
                                                       p(Tt(of)), p(Tt(oi)), len(of), p(Tt(ref)), nsel, p(Tt(sel)), int(what), p(best), p(status), s))
    torch.cuda.synchronize()
    gp = d_pts.cpu().numpy().view(MAP_POINT_DTYPE).reshape(-1)
    gd = d_pd.cpu().numpy()
    best, status = best.cpu().numpy(), status.cpu().numpy()
    untouched = bool(np.all(best[nsel:] == -9) and np.all(status[nsel:] == -9))
    chosen = np.zeros(len(allpts), bool)
    chosen[sel] = True
    untouched = untouched and gp[~chosen].tobytes() == pts[~chosen].tobytes() and gd[~chosen].tobytes() == pd[~chosen].tobytes()
    out = []
    for k, c in enumerate(cases):
        a, b = poff[k], poff[k] + len(c.points)
        out.append((gp[a:b], gd[a:b], best[cut[k]:cut[k + 1]], status[cut[k]:cut[k + 1]]))
    return out, untouched
