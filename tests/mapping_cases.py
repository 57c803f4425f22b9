"""Constructed key frames for CreateNewMapPoints (pilotguru_amd/csrc/mapping.hip, k_cnm_*) and the runners that put them through
the plain reference (tests/mapping_reference.py), the single-call ABI and the batched device form.  A helper module (no tests):
tests/test_create_new_map_points.py uses it.

A scene is KF1 at the world origin and neighbours with chosen poses, all with K = [[f, 0, cx], [0, f, cy], [0, 0, 1]], and 3D
points projected into every key frame (in double, rounded to float) with a chosen pixel error and octave per observation.
Point j has its own random descriptor; its observations carry it at a small Hamming distance and sit in vocabulary node
j % nodes, so the matcher sees several candidates per node.  The poses and point sets place observations on both sides of the
parallax limits, in front of and behind each camera, inside and outside both chi-square limits and both scale-ratio bounds."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_reference as MR  # noqa: E402
import triangulation_reference as TR  # noqa: E402
from matcher_cases import SF, _fv, keys, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, kf_pose  # noqa: E402

f32 = np.float32
S2 = TR.level_sigma2(SF)
NLEVELS = 8
SCALE = float(SF[1])


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, C, f, cx, cy):
    """A KF_POSE_DTYPE record of a camera at centre C with world-to-camera rotation R: Tcw = [R | -R C], Ow = -R^T t (float)."""
    R = np.asarray(R, np.float64)
    t = -R @ np.asarray(C, np.float64)
    Rf, tf = R.astype(np.float32), t.astype(np.float32)
    Ow = (-(Rf.astype(np.float64).T @ tf.astype(np.float64))).astype(np.float32)    # SetPose: Ow = -Rwc*tcw
    return kf_pose(np.hstack([Rf, tf[:, None]]), Ow, f, f, cx, cy)


def project(P, X):
    T = np.asarray(P["Tcw"], np.float64).reshape(3, 4)
    c = T[:, :3] @ X + T[:, 3]
    return float(P["fx"]) * c[0] / c[2] + float(P["cx"]), float(P["fy"]) * c[1] / c[2] + float(P["cy"]), c[2]


def scene(seed, w=640, h=480, nneigh=5, npts=300, nodes=60, focal=500.0, rotations=True, far=True):
    """KF1 + nneigh neighbours over npts points; returns (KF1, neighbours) dicts as mapping_reference takes them."""
    rng = np.random.RandomState(seed)
    cx, cy = w / 2.0, h / 2.0
    P1 = pose(np.eye(3), (0, 0, 0), focal, cx, cy)
    poses = []
    for s in range(nneigh):
        kind = s % 5
        if kind == 0:
            R, C = np.eye(3), (0.3 + 0.1 * s, 0.02 * rng.randn(), 0.01 * rng.randn())              # sideways
        elif kind == 1:
            R, C = rot(0.02 * rng.randn(), 0.15, 0.01), (0.6, 0.05, 0.1)                       # sideways + yaw
        elif kind == 2:
            R, C = np.eye(3), (3.0, 0.0, 6.5)                                                   # ahead: the far points are behind it
        elif kind == 3:
            R, C = np.eye(3), (3.0, 0.0, -6.0)                                                  # behind: sees the points behind KF1
        else:
            R, C = np.eye(3), (1e-3, 0.0, 0.0)                                                  # tiny baseline: skipped
        poses.append(pose(R, C, focal, cx, cy))
    # points: mostly at depth 2-8 in front of KF1, some very far (parallax), some wide (behind the yawed camera)
    X = np.stack([rng.uniform(-3, 3, npts), rng.uniform(-2, 2, npts), rng.uniform(2, 8, npts)], 1)
    X[-npts // 10:, 2] = -rng.uniform(1, 4, npts // 10)                                        # behind KF1
    if far:
        X[: npts // 8, 2] = rng.uniform(300, 3000, npts // 8)
        X[npts // 8: npts // 6, :] = np.stack([rng.uniform(-12, -4, npts // 6 - npts // 8), rng.uniform(-1, 1, npts // 6 - npts // 8),
                                               rng.uniform(1.5, 4, npts // 6 - npts // 8)], 1)
    D = rand_desc(rng, npts)

    def observe(P, drop_p):
        ks, ds, nd = [], [], []
        for j in range(npts):
            u, v, z = project(P, X[j])
            if rng.rand() < drop_p or not np.isfinite(u) or abs(u) > 1e5 or abs(v) > 1e5:
                continue
            err = rng.choice([0.0, 0.5, 1.5, 3.0, 6.0], p=[0.4, 0.25, 0.15, 0.1, 0.1])          # px of reprojection error
            a = rng.uniform(0, 2 * math.pi)
            o = int(rng.choice([0, 0, 0, 0, 1, 2, 4, 7]))
            ks.append((u + err * math.cos(a), v + err * math.sin(a), o))
            d = D[j].copy()
            for b in rng.choice(256, int(rng.randint(0, 12)), replace=False):
                d[b // 8] ^= 1 << (b % 8)
            ds.append(d)
            nd.append(j % nodes)
        order = rng.permutation(len(ks))
        k = keys([ks[i][0] for i in order], [ks[i][1] for i in order], octave=np.array([ks[i][2] for i in order], np.int32))
        return k, np.array([ds[i] for i in order], np.uint8).reshape(-1, 32), [nd[i] for i in order]

    def kf(P, drop_p, median=None):
        k, d, nd = observe(P, drop_p)
        out = dict(k=k, d=d, fv=_fv(nd), h=(rng.rand(len(k)) < 0.1).astype(np.uint8), pose=P)
        if median is not None:
            out["median"] = f32(median)
        return out
    KF1 = kf(P1, 0.1)
    neigh = [kf(P, 0.2, median=(4.0 if s % 5 != 4 else 0.2)) for s, P in enumerate(poses)]
    return KF1, neigh


def ride_scene(keys_, descs, fvs, frames, w, h, dx, dy, focal=500.0, seed=0):
    """Key frames of synth_ride(..., dx, dy): frame k is the scene window moved by (k dx, k dy) px, i.e. a camera moved by
    (k dx / f, k dy / f, 0) over a fronto-parallel plane at depth 1 (R = I, median depth 1).  frames[0] is KF1, the rest
    its neighbours in the given order; keys_ / descs / fvs are indexed by frame.  Masks are random (10 %)."""
    rng = np.random.RandomState(seed)
    out = []
    for f in frames:
        P = pose(np.eye(3), (f * dx / focal, f * dy / focal, 0.0), focal, w / 2.0, h / 2.0)
        k = np.ascontiguousarray(keys_[f], KEYPOINT_DTYPE)
        out.append(dict(k=k, d=np.ascontiguousarray(descs[f], np.uint8).reshape(-1, 32), fv=fvs[f], pose=P, median=f32(1.0),
                        h=(rng.rand(len(k)) < 0.1).astype(np.uint8)))
    return out[0], out[1:]


def same_point_lists(a, b):
    """Two point lists equal bit for bit: (slot, idx1, idx2, pos, normal, min, max)."""
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if tuple(int(x) for x in p[:3]) != tuple(int(x) for x in q[:3]):
            return False
        for x, y in zip(p[3:], q[3:]):
            if np.asarray(x, np.float32).tobytes() != np.asarray(y, np.float32).tobytes():
                return False
    return True


def run_reference(KF1, neigh, rules=MR.REFERENCE, hits=None, pair_hook=None):
    return MR.create_new_map_points(KF1, neigh, SF, S2, NLEVELS, f32(SCALE), rules, hits, pair_hook)


def per_pair_results(KF1, neigh):
    """{slot: (matches12, {idx1: triangulate() result})} of every searched pair, each matched with KF1's ENTRY mask."""
    per = {}
    for s, K2 in enumerate(neigh):
        F = MR.compute_f12(KF1["pose"], K2["pose"])
        ep = MR.epipole(KF1["pose"], K2["pose"])
        _, _, Ow1 = MR._pose(KF1["pose"])
        _, _, Ow2 = MR._pose(K2["pose"])
        base = f32(MR.normd([f32(Ow2[i] - Ow1[i]) for i in range(3)]))
        if float(f32(base / f32(K2["median"]))) < 0.01:
            continue
        _, m12 = TR.search_for_triangulation(KF1["k"], KF1["d"], KF1["h"], KF1["fv"], K2["k"], K2["d"], K2["h"], K2["fv"], F, ep,
                                             SF, S2, False)
        res = {}
        for i in np.nonzero(m12 >= 0)[0]:
            res[int(i)] = MR.triangulate(KF1["k"][i], K2["k"][int(m12[i])], KF1["pose"], K2["pose"], SF, S2, NLEVELS,
                                         f32(f32(1.5) * f32(SCALE)))
        per[s] = (m12, res)
    return per


def parallel_first_success(KF1, neigh):
    """The parallel form: every pair matched with KF1's ENTRY mask and triangulated on its own (the reference's per-pair
    results), then the first success per idx1 in neighbour order, written out neighbour by neighbour in ascending idx1."""
    per = per_pair_results(KF1, neigh)
    win = {}
    for s in sorted(per):
        m12, res = per[s]
        for i, r in res.items():
            if r is not None and i not in win:
                win[i] = s
    pts = []
    for s in sorted(per):
        m12, res = per[s]
        for i in sorted(i for i, w in win.items() if w == s):
            pts.append((s, i, int(m12[i])) + tuple(res[i]))
    return pts


# ---------------------------------------------------------------- GPU
class KeyFrameArrays:
    """What the mirror reads from a key frame: ext, N, mvKeysUndistorted, mDescriptors."""

    def __init__(self, ext, k, d):
        self.ext = ext
        self.mvKeys = self.mvKeysUndistorted = np.ascontiguousarray(k, KEYPOINT_DTYPE)
        self.mDescriptors = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
        self.N = len(k)


def gpu_points(pts):
    return [(int(p["neighbour"]), int(p["idx1"]), int(p["idx2"]), p["pos"].copy(), p["normal"].copy(), f32(p["min_distance"]),
             f32(p["max_distance"])) for p in pts]


def run_gpu(KF1, neigh, ext):
    import pilotguru_amd as pg
    K1 = KeyFrameArrays(ext, KF1["k"], KF1["d"])
    Ks = [KeyFrameArrays(ext, K["k"], K["d"]) for K in neigh]
    pts, count, F12, ep, h = pg.LocalMapping.CreateNewMapPoints(K1, Ks, KF1["fv"], [K["fv"] for K in neigh], KF1["pose"],
                                                                [K["pose"] for K in neigh], [K["median"] for K in neigh],
                                                                KF1["h"], [K["h"] for K in neigh])
    return gpu_points(pts), list(count), F12, ep, h


def run_gpu_batched(problems, ext, extra=3, M=None, device_fv=None):
    """Every problem (KF1, neighbours) in ONE pgorb_create_new_map_points_batch_device call: frames laid out problem by problem
    (KF1 first, then its neighbours), cap = largest n + extra with NaN keypoints and 0xFF descriptors past n, masks set past n.
    Returns per problem (points, count, F12, epipole, has_point1_out)."""
    import ctypes as C
    import torch
    L, hd = ext._L, ext._h
    frames, kf1, neigh_idx = [], [], []
    for KF1, neigh in problems:
        kf1.append(len(frames)); frames.append(KF1)
        neigh_idx.append(list(range(len(frames), len(frames) + len(neigh)))); frames += neigh
    B, nkf = len(frames), len(problems)
    M = M or max(len(n) for _, n in problems)
    cap = max(len(f["k"]) for f in frames) + extra
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["angle"] = np.nan, np.nan, np.nan
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    hp = np.ones((B, cap), np.uint8)
    fvn = np.full((B, cap), 0xFFFFFFFF, np.uint32); fvs = np.zeros((B, cap + 1), np.int32); fvf = np.full((B, cap), 0xFFFFFFFF, np.uint32)
    n = np.zeros(B, np.int32); nfv = np.zeros(B, np.int32)
    poses = np.zeros(B, KF_POSE_DTYPE)
    for f, F in enumerate(frames):
        k, d, fv = F["k"], F["d"], F["fv"]
        n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d; hp[f, :len(k)] = F["h"]
        nfv[f] = len(fv[0]); fvn[f, :len(fv[0])] = fv[0]; fvs[f, :len(fv[1])] = fv[1]; fvf[f, :len(fv[2])] = fv[2]
        poses[f] = F["pose"]
    nb = np.zeros((nkf, M), np.int32); nn = np.zeros(nkf, np.int32); md = np.zeros((nkf, M), np.float32)
    for k, (KF1, neigh) in enumerate(problems):
        nn[k] = len(neigh)
        for s, K in enumerate(neigh):
            nb[k, s] = neigh_idx[k][s]; md[k, s] = K["median"]
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dk = Tt(kp.view(np.uint8).reshape(B, cap, 28))
    if device_fv is not None:
        fvn_t, fvs_t, fvf_t, nfv_t = device_fv(frames, cap)
    else:
        fvn_t, fvs_t, fvf_t, nfv_t = Tt(fvn), Tt(fvs), Tt(fvf), Tt(nfv)
    pts = torch.full((nkf, cap * 44), 0x7F, dtype=torch.uint8, device="cuda")
    npt = torch.full((nkf,), -9, dtype=torch.int32, device="cuda")
    cnt = torch.full((nkf, M), -9, dtype=torch.int32, device="cuda")
    F12 = torch.full((nkf, M, 9), 7.0, dtype=torch.float32, device="cuda")
    ep = torch.full((nkf, M, 2), 7.0, dtype=torch.float32, device="cuda")
    hout = torch.full((nkf, cap), 9, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_create_new_map_points_batch_device(hd, p(dk), p(Tt(ds)), p(Tt(n)), cap, p(fvn_t), p(fvs_t), p(fvf_t), p(nfv_t),
                                                          p(Tt(poses.view(np.uint8))), p(Tt(hp)), p(Tt(np.array(kf1, np.int32))), nkf,
                                                          p(Tt(nb)), p(Tt(nn)), M, p(Tt(md)), p(pts), p(npt), p(cnt), p(F12), p(ep), p(hout), s))
    torch.cuda.synchronize()
    import pilotguru_amd as pg
    ph = pts.cpu().numpy().view(pg.NEW_MAP_POINT_DTYPE).reshape(nkf, cap)
    out = []
    for k, (KF1, neigh) in enumerate(problems):
        npk = int(npt[k])
        out.append((gpu_points(ph[k, :npk]), list(cnt[k, :len(neigh)].cpu().numpy()), F12[k, :len(neigh)].cpu().numpy().reshape(-1, 3, 3),
                    ep[k, :len(neigh)].cpu().numpy(), hout[k, :len(KF1["k"])].cpu().numpy(), cnt[k].cpu().numpy(), n))
    return out
