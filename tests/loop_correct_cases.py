"""Cases for loop correction (tests/test_loop_correction.py): maps in plain dicts of numpy arrays in the layouts of include/pgorb.h,
constructed cases by name, seeded random worlds, two large cases, and the runners (reference, host form, device form).

A loop case holds nkf, octaves[f], pose [nkf], cur_kf, scw, list, kf_order (or None), kf_point[f], npoints, points, point_bad,
obs_start / obs_frame / obs_idx, ref_obs, ref_kf.  A map case holds nkf, pose, pose_gba, kf_done, parent, kf_origin, kf_bad,
npoints, points, pos_gba, point_done, point_bad, ref_kf."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_correct_reference as LR  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, MAP_POINT_DTYPE, SIM3D_DTYPE  # noqa: E402

f32, f64 = np.float32, np.float64
LOOP_KEYS = ("has_corrected", "corrected", "has_non_corrected", "non_corrected", "pose_out", "points", "corrected_by", "point_ref_kf", "info")
MAP_KEYS = ("pose_out", "kf_updated", "points", "point_updated", "info")
SENT = 0xA5                                   # every output byte before a call


# ---------------------------------------------------------------- poses
def rot(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)).astype(f32)


def pose(R, t, Ow=None):
    """a KF_POSE_DTYPE record; Ow = SetPose's unless given (the library reads it as given)"""
    P = np.zeros((), KF_POSE_DTYPE)
    T = np.concatenate([np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3, 1)], 1).reshape(12)
    P["Tcw"] = T
    P["Ow"] = LR.set_pose_ow(T) if Ow is None else Ow
    P["fx"], P["fy"], P["cx"], P["cy"] = 500.0, 510.0, 320.25, 240.5
    P["invfx"], P["invfy"] = f32(1) / f32(500.0), f32(1) / f32(510.0)
    return P


def sim3(q, t, s):
    S = np.zeros((), SIM3D_DTYPE)
    S["r"], S["t"], S["s"] = q, t, s
    return S


def sim3_near(P, s, rng, jitter=0.05, norm=1.0):
    """a Sim3 close to pose P's, with scale s and a quaternion of norm `norm` (g2o never renormalises)"""
    T = np.asarray(P["Tcw"], f32).reshape(3, 4).astype(f64)
    R = T[:, :3] @ rot(rng.normal(size=3), jitter * 60).astype(f64)
    q = LR.quat_from_matrix(R) * norm
    return sim3(q, s * T[:, 3] + rng.normal(size=3) * jitter, s)


# ---------------------------------------------------------------- building a loop case
def loop_case(name, poses, cur, scw, lst, points, order=None, hole=()):
    """points: dicts(pos, holders, observers (default: the holders), ref (a key frame; default: the first observer in address
    order), bad, octave, normal).  An observer gets a fresh keypoint whose slot holds the point only if it is a holder; a holder
    that does not observe gets a slot without an observation.  hole: key frames that start with an empty slot."""
    nkf = len(poses)
    rank = (lambda f: f) if order is None else (lambda f: int(order[f]))
    slots, octv = [[-1] if f in hole else [] for f in range(nkf)], [[0] if f in hole else [] for f in range(nkf)]
    n = len(points)
    pts, bad = np.zeros(n, MAP_POINT_DTYPE), np.zeros(n, np.uint8)
    st, of, oi, ro, rk = [0], [], [], [], []
    for p, d in enumerate(points):
        holders = list(d["holders"])
        obs = sorted(d.get("observers", holders), key=rank)
        pts[p]["pos"], pts[p]["normal"] = d["pos"], d.get("normal", (0.1, 0.2, 0.3))
        pts[p]["min_distance"], pts[p]["max_distance"] = d.get("min_d", 0.5), d.get("max_d", 9.0)
        bad[p] = d.get("bad", False)
        for f in obs:
            of.append(f)
            oi.append(len(slots[f]))
            slots[f].append(p if f in holders else -1)
            octv[f].append(d.get("octave", p % 8))
        for f in holders:
            if f not in obs:
                slots[f].append(p)
                octv[f].append(0)
        st.append(len(of))
        ref = d.get("ref", obs[0] if obs else -1)
        ro.append(obs.index(ref) if ref in obs else 0)
        rk.append(d.get("ref_kf", ref))
    return dict(name=name, nkf=nkf, octaves=[np.array(o, np.int32) for o in octv], pose=np.array(poses, KF_POSE_DTYPE), cur_kf=cur,
                scw=np.array(scw, SIM3D_DTYPE).reshape(()), list=np.array(lst, np.int32), kf_order=None if order is None else np.array(order, np.int32),
                kf_point=[np.array(s, np.int32) for s in slots], npoints=n, points=pts, point_bad=bad, obs_start=np.array(st, np.int32),
                obs_frame=np.array(of, np.int32), obs_idx=np.array(oi, np.int32), ref_obs=np.array(ro, np.int32), ref_kf=np.array(rk, np.int32))


def _ring(nkf, rng, spread=25.0):
    """key frames looking at the origin region from a ring, with moderate rotations"""
    out = []
    for f in range(nkf):
        R = rot(rng.normal(size=3), rng.uniform(-spread, spread)) @ rot((0, 1, 0), 9.0 * f)
        out.append(pose(R, rng.normal(size=3) * 0.6 + (0, 0, 4.0)))
    return out


def loop_cases():
    rng = np.random.RandomState(11)
    out = []
    P = _ring(6, rng)
    order = [4, 3, 5, 0, 1, 2]                                     # rank(3) = 0 < rank(1) = 3 < rank(2) = 5
    shared = [dict(pos=(0.3, -0.2, 0.8), holders=[1, 3], ref=1, octave=2), dict(pos=(-0.5, 0.4, 1.1), holders=[1, 2, 3], ref=2, octave=7),
              dict(pos=(0.1, 0.1, 0.5), holders=[0, 5], ref=0, octave=0), dict(pos=(1.0, 0.2, -0.4), holders=[2], octave=3),
              dict(pos=(0.7, 0.7, 0.7), holders=[4, 1], ref=4, octave=1), dict(pos=(0.2, 0.9, 0.1), holders=[3, 2], bad=True)]
    for nm, s in (("address_vs_index", 1.1), ("scale_half", 0.5), ("scale_two", 2.0)):
        out.append(loop_case(nm, P, 2, sim3_near(P[2], s, rng), [1, 3, 4], shared, order, hole=(1,)))
    out.append(loop_case("index_order", P, 2, sim3_near(P[2], 0.9, rng), [3, 1], shared))
    out.append(loop_case("unnormalised_scw", P, 2, sim3_near(P[2], 1.3, rng, norm=1.0 + 3e-7), [1, 3], shared, order))
    out.append(loop_case("padded_row", P, 2, sim3_near(P[2], 1.2, rng), [3, 1, -1, -1, 2, 6, 99, 1, -7], shared, order))
    out.append(loop_case("cur_alone", P, 2, sim3_near(P[2], 0.8, rng), [], shared, order))
    # inconsistent slots: key frame 0 (rank 0) and 5 (rank 1) are members and observe point 0, but only 5 holds it: 5 corrects it after
    # 0's SetPose.  Point 1 sits in a slot of 5 without any observation; point 2 is observed by the non-member 4 too.
    o2 = [0, 5, 4, 3, 2, 1]
    inc = [dict(pos=(0.4, 0.1, 0.9), holders=[5], observers=[0, 5, 3], ref=5, octave=1), dict(pos=(0.2, 0.3, 0.4), holders=[5], observers=[]),
           dict(pos=(-0.3, 0.2, 0.6), holders=[0, 5], observers=[0, 4, 5], ref=4, octave=5),
           dict(pos=(0.9, -0.1, 0.2), holders=[3], observers=[0, 3, 5], ref=0, ref_kf=2, octave=6)]
    out.append(loop_case("inconsistent_slots", P, 5, sim3_near(P[5], 1.4, rng), [0, 3], inc, o2))
    # half turns: relative and absolute rotations past 120 degrees about each axis take Quaterniond(R)'s three non-trace branches
    H = [pose(np.eye(3, dtype=f32), (0.1, 0.2, 3.0))] + [pose(rot(ax, 170.0), (0.2 * i, -0.1, 3.5)) for i, ax in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1)))]
    hp = [dict(pos=(0.1 * p, 0.2, 0.3 + 0.1 * p), holders=[p % 4, (p + 1) % 4], octave=p) for p in range(6)]
    out.append(loop_case("half_turns", H, 0, sim3_near(H[0], 1.0, rng), [1, 2, 3], hp, [2, 0, 3, 1]))
    # a point over PGORB_MP_MAX_OBS: 513 observers, held by the current key frame and one more
    nbig = LR.MAX_OBS + 3
    B = [pose(rot((0, 1, 0), 0.05 * f), (0.01 * f, 0.0, 4.0)) for f in range(nbig)]
    big = [dict(pos=(0.2, 0.1, 0.5), holders=[0, 1], observers=list(range(LR.MAX_OBS + 1)), ref=0, octave=2),
           dict(pos=(0.3, 0.3, 0.6), holders=[1, 2], octave=4)]
    out.append(loop_case("over_max_obs", B, 0, sim3_near(B[0], 1.05, rng), [1, 2, 7], big))
    return out


# ---------------------------------------------------------------- building a map case
def map_case(name, poses, gba, done, parent, origin, bad, points, pos_gba, point_done, point_bad, ref_kf):
    n = len(points)
    pts = np.zeros(n, MAP_POINT_DTYPE)
    pts["pos"] = np.asarray(points, f32).reshape(n, 3)
    pts["normal"], pts["min_distance"], pts["max_distance"] = (0.5, 0.25, 0.125), 0.75, 7.5
    return dict(name=name, nkf=len(poses), pose=np.array(poses, KF_POSE_DTYPE), pose_gba=np.array(gba, KF_POSE_DTYPE), kf_done=np.array(done, np.uint8),
                parent=np.array(parent, np.int32), kf_origin=np.array(origin, np.uint8), kf_bad=None if bad is None else np.array(bad, np.uint8),
                npoints=n, points=pts, pos_gba=np.asarray(pos_gba, f32).reshape(n, 3), point_done=np.array(point_done, np.uint8),
                point_bad=None if point_bad is None else np.array(point_bad, np.uint8), ref_kf=np.array(ref_kf, np.int32))


def _adjusted(P, rng, amount=4.0):
    """what a bundle adjustment could leave: the pose moved a little, Ow by SetPose"""
    T = np.asarray(P["Tcw"], f32).reshape(3, 4)
    return pose(rot(rng.normal(size=3), amount) @ T[:, :3], T[:, 3] + rng.normal(size=3).astype(f32) * 0.05)


def _map_from(name, rng, nkf, parent, done, origin, bad=None, npts=12, point_bad=None, stale_ow=()):
    P = _ring(nkf, rng, 60.0)
    for k in stale_ow:                                              # Ow as given, not SetPose's: the library must not recompute it
        P[k]["Ow"] = P[k]["Ow"] + f32(0.01)
    G = [_adjusted(p, rng) for p in P]
    pts = rng.normal(size=(npts, 3)) * 2.0
    return map_case(name, P, G, done, parent, origin, bad, pts, pts + rng.normal(size=(npts, 3)) * 0.02, [p % 3 == 0 for p in range(npts)], point_bad,
                    [(p * 5) % (nkf + 1) - 1 for p in range(npts)])


def map_cases():
    rng = np.random.RandomState(23)
    out = []
    # 0 (origin, done) - 1 - 2 (both not done) - 3 (done) - 4 (not done); 5 done but its chain ends at no origin; 6 hangs under 5
    out.append(_map_from("chain", rng, 7, [-1, 0, 1, 2, 3, -1, 5], [1, 0, 0, 1, 0, 1, 0], [1, 0, 0, 0, 0, 0, 0], npts=14, stale_ow=(1,)))
    # the origin is not done: 1 (not done) has no adjusted ancestor, 2 (done) and 3 (not done, under 2) have
    out.append(_map_from("origin_not_done", rng, 5, [-1, 0, 1, 2, 0], [0, 0, 1, 0, 0], [1, 0, 0, 0, 0]))
    # a bad key frame in the chain: 2 is bad, 3 under it is not visited; 4 is bad itself; two origins
    out.append(_map_from("bad_in_chain", rng, 7, [-1, 0, 1, 2, 0, -1, 5], [1, 0, 1, 1, 1, 1, 0], [1, 0, 0, 0, 0, 1, 0], bad=[0, 0, 1, 0, 1, 0, 0],
                         point_bad=[p == 1 for p in range(12)]))
    out.append(_map_from("all_done", rng, 4, [-1, 0, 0, 2], [1, 1, 1, 1], [1, 0, 0, 0]))
    out.append(_map_from("nothing_done", rng, 4, [-1, 0, 0, 2], [0, 0, 0, 0], [1, 0, 0, 0]))
    c = _map_from("cycle", rng, 6, [-1, 0, 3, 4, 2, 5], [1, 0, 1, 0, 1, 1], [1, 0, 0, 0, 0, 0])          # 2 -> 3 -> 4 -> 2, and 5 its own parent
    c["device_only"] = True                                         # the single call refuses a parent cycle
    out.append(c)
    return out


# ---------------------------------------------------------------- seeded random worlds: (loop case, map case) on one map
def random_world(seed):
    rng = np.random.RandomState(1000 + seed)
    nkf = int(rng.randint(4, 13))
    P = _ring(nkf, rng, 50.0)
    order = [int(x) for x in rng.permutation(nkf)] if seed % 4 else None
    npts = int(rng.randint(8, 49))
    pts = []
    budget = [16] * nkf
    for p in range(npts):
        free = [f for f in range(nkf) if budget[f] > 0]
        if not free:
            break
        k = min(int(rng.randint(1, 5)), len(free))
        holders = [int(x) for x in rng.choice(free, k, replace=False)]
        for f in holders:
            budget[f] -= 1
        pts.append(dict(pos=rng.normal(size=3) * 1.5, holders=holders, ref=holders[int(rng.randint(k))], octave=int(rng.randint(8)),
                        bad=bool(rng.rand() < 0.08)))
    cur = int(rng.randint(nkf))
    lst = [int(x) for x in rng.choice(nkf, int(rng.randint(1, nkf)), replace=False)] + ([-1] * int(rng.randint(3)) if seed % 3 == 0 else [])
    s = float(rng.choice([0.5, 0.8, 1.0, 1.25, 2.0]))
    lc = loop_case("random_loop_%d" % seed, P, cur, sim3_near(P[cur], s, rng), lst, pts, order)
    parent = [-1] + [int(rng.randint(0, k)) for k in range(1, nkf)]
    origin = [1] + [0] * (nkf - 1)
    if seed % 5 == 0 and nkf > 5:                                   # a second tree with its own origin
        parent[nkf - 2], origin[nkf - 2] = -1, 1
    done = [int(rng.rand() < 0.45) for _ in range(nkf)]
    done[0] = int(seed % 7 != 0)                                    # now and then the origin itself was not adjusted
    bad = [int(k and rng.rand() < 0.08) for k in range(nkf)]
    n = lc["npoints"]
    G = [_adjusted(p, rng) for p in P]
    pos = np.array(lc["points"]["pos"], f32)
    mc = map_case("random_map_%d" % seed, P, G, done, parent, origin, bad if any(bad) or seed % 2 else None, pos,
                  pos + rng.normal(size=(n, 3)).astype(f32) * 0.02, [int(rng.rand() < 0.5) for _ in range(n)], lc["point_bad"],
                  [int(rng.randint(-1, nkf)) if rng.rand() < 0.1 else int(r) for r in lc["ref_kf"]])
    return lc, mc


def world_facts(lc, mc, el, em):
    """what the coverage test counts, by the reference alone"""
    members = set(LR.members_of(lc))
    rank = lambda f: LR.rank_of(lc, f)
    holders = {}
    for f in members:
        for p in lc["kf_point"][f]:
            if p >= 0 and not lc["point_bad"][p]:
                holders.setdefault(int(p), set()).add(f)
    first_not_index = any(len(h) >= 2 and min(h, key=rank) != min(h) for h in holders.values())
    upd, nkf = em["kf_updated"], mc["nkf"]
    rec = [bool(upd[k]) and not mc["kf_done"][k] for k in range(nkf)]
    chain2 = any(rec[k] and 0 <= mc["parent"][k] < nkf and rec[mc["parent"][k]] for k in range(nkf))
    not_visited = not upd.all()
    pb = mc["point_bad"] if mc["point_bad"] is not None else np.zeros(mc["npoints"], np.uint8)
    live = [p for p in range(mc["npoints"]) if not pb[p] and not mc["point_done"][p] and mc["ref_kf"][p] >= 0]
    moved = any(upd[mc["ref_kf"][p]] for p in live)
    kept = any(not upd[mc["ref_kf"][p]] for p in live)
    return dict(first_not_index=first_not_index, chain2=chain2, not_visited=not_visited, ref_both=moved and kept)


# ---------------------------------------------------------------- the large cases
def chain300():
    """a spanning-tree chain of 300 key frames that were not adjusted under one adjusted origin, and 4000 points"""
    rng = np.random.RandomState(5)
    nkf, npts = 301, 4000
    P = [pose(rot((0.1, 1, 0.05), 1.7 * f) @ rot((1, 0, 0), 3.0 * np.sin(f)), (0.02 * f, 0.01 * np.cos(f), 4.0 + 0.01 * f)) for f in range(nkf)]
    G = [_adjusted(P[0], rng)] + P[1:]
    pts = rng.normal(size=(npts, 3)) * 3.0
    return map_case("chain300", P, G, [1] + [0] * (nkf - 1), [-1] + list(range(nkf - 1)), [1] + [0] * (nkf - 1), None, pts,
                    pts + 0.01, [p % 17 == 0 for p in range(npts)], None, [p % nkf for p in range(npts)])


def claim64x256():
    """64 members x up to 256 slots, every point held by up to 8 of them: 2048 points"""
    rng = np.random.RandomState(6)
    nkf, per, nslots = 66, 8, 256
    P = _ring(nkf, rng, 40.0)
    order = [int(x) for x in rng.permutation(nkf)]
    npts = 64 * nslots // per
    deck = []
    for _ in range(nslots // per):                                  # 32 rounds; in each every member holds 8 of the round's 64 points
        perm = [rng.permutation(64) for _ in range(per)]
        for j in range(64):
            deck.append(sorted({int(perm[k][j]) for k in range(per)}))
    pts = [dict(pos=rng.normal(size=3) * 1.5, holders=h, ref=h[int(rng.randint(len(h)))], octave=p % 8) for p, h in enumerate(deck[:npts])]
    return loop_case("claim64x256", P, 63, sim3_near(P[63], 1.15, rng), list(range(63)), pts, order)


# ---------------------------------------------------------------- comparing
def same(a, b, keys):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def diff(a, b, keys):
    out = []
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.tobytes() != y.tobytes():
            if x.shape == y.shape and x.dtype == y.dtype and x.ndim:
                w = [i for i in range(len(x)) if x[i].tobytes() != y[i].tobytes()]
                out.append("%s at %s: %s != %s" % (k, w[:6], x[w[0]], y[w[0]]))
            else:
                out.append("%s: %s != %s" % (k, x, y))
    return "; ".join(out)


# ---------------------------------------------------------------- runners
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _sent(n, dtype):
    return np.frombuffer(bytes([SENT]) * (max(n, 1) * np.dtype(dtype).itemsize), dtype).copy()


def run_host_loop(c, ext):
    """the single call through the C ABI, the outputs starting as the sentinel"""
    nkf, n = c["nkf"], c["npoints"]
    ks = []
    kps, slots = (C.c_void_p * nkf)(), (C.c_void_p * nkf)()
    for f in range(nkf):
        k = np.zeros(max(len(c["octaves"][f]), 1), KEYPOINT_DTYPE)
        k["octave"][:len(c["octaves"][f])] = c["octaves"][f]
        ks.append(k)
        kps[f], slots[f] = k.ctypes.data, c["kf_point"][f].ctypes.data if len(c["kf_point"][f]) else None
    nk = np.array([len(s) for s in c["kf_point"]], np.int32)
    pts = c["points"].copy()
    out = dict(has_corrected=_sent(nkf, np.uint8), corrected=_sent(nkf, SIM3D_DTYPE), has_non_corrected=_sent(nkf, np.uint8),
               non_corrected=_sent(nkf, SIM3D_DTYPE), pose_out=_sent(nkf, KF_POSE_DTYPE), corrected_by=_sent(n, np.int32),
               point_ref_kf=_sent(n, np.int32), info=_sent(LR.LC_INFO, np.int32))
    one = np.zeros(1, np.int32)
    lst = c["list"] if len(c["list"]) else one
    rc = ext._L.pgorb_correct_loop_poses(
        ext._h, nkf, kps, _p(nk), _p(c["pose"]), int(c["cur_kf"]), _p(c["scw"].reshape(1)), len(c["list"]), _p(lst),
        None if c["kf_order"] is None else _p(c["kf_order"]), slots, n, _p(pts), _p(c["point_bad"]), _p(c["obs_start"]),
        _p(c["obs_frame"] if len(c["obs_frame"]) else one), _p(c["obs_idx"] if len(c["obs_idx"]) else one), _p(c["ref_obs"]), _p(c["ref_kf"]),
        _p(out["has_corrected"]), _p(out["corrected"]), _p(out["has_non_corrected"]), _p(out["non_corrected"]), _p(out["pose_out"]),
        _p(out["corrected_by"]), _p(out["point_ref_kf"]), _p(out["info"]))
    out = {k: v[:n] if k in ("corrected_by", "point_ref_kf") else v for k, v in out.items()}
    out["points"], out["ret"] = pts, rc
    return out


def loop_device_arrays(c, stream=None):
    """the case on the device in the batch layout: a dict of torch tensors, the outputs holding the sentinel"""
    import torch
    nkf, n = c["nkf"], c["npoints"]
    cap = max(1, max(len(s) for s in c["kf_point"]))
    K, S = np.zeros((nkf, cap), KEYPOINT_DTYPE), np.full((nkf, cap), -1, np.int32)
    for f in range(nkf):
        m = len(c["kf_point"][f])
        K["octave"][f, :m], S[f, :m] = c["octaves"][f], c["kf_point"][f]
    up = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()
    upi = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1).copy()).cuda()
    sent = lambda nbytes: torch.full((max(nbytes, 1),), SENT, dtype=torch.uint8, device="cuda")
    D = dict(cap=cap, kps=up(K), n=upi([len(s) for s in c["kf_point"]]), pose=up(c["pose"]), scw=up(c["scw"].reshape(1)),
             list=upi(c["list"] if len(c["list"]) else [0]), order=None if c["kf_order"] is None else upi(c["kf_order"]), slots=upi(S),
             pts=up(c["points"] if n else np.zeros(1, MAP_POINT_DTYPE)), pb=up(c["point_bad"] if n else np.zeros(1, np.uint8)), os=upi(c["obs_start"]),
             of=upi(c["obs_frame"] if len(c["obs_frame"]) else [0]), oi=upi(c["obs_idx"] if len(c["obs_idx"]) else [0]),
             ro=upi(c["ref_obs"] if n else [0]), rk=upi(c["ref_kf"] if n else [0]),
             has_corrected=sent(nkf), corrected=sent(nkf * 64), has_non_corrected=sent(nkf), non_corrected=sent(nkf * 64),
             pose_out=sent(nkf * KF_POSE_DTYPE.itemsize), corrected_by=sent(n * 4), point_ref_kf=sent(n * 4), info=sent(LR.LC_INFO * 4))
    return D


def run_device_loop(c, ext, stream=None, D=None, list_count=None, download=True):
    """the device form on resident arrays; returns (outputs downloaded, the device arrays); download=False: enqueued only"""
    import torch
    D = loop_device_arrays(c) if D is None else D
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        rc = ext._L.pgorb_correct_loop_poses_device(
            ext._h, q(D["kps"]), q(D["n"]), c["nkf"], D["cap"], q(D["pose"]), int(c["cur_kf"]), q(D["scw"]), len(c["list"]), q(D["list"]),
            q(list_count), q(D["order"]), q(D["slots"]), c["npoints"], q(D["pts"]), q(D["pb"]), q(D["os"]), q(D["of"]), q(D["oi"]),
            len(c["obs_frame"]), q(D["ro"]), q(D["rk"]), q(D["has_corrected"]), q(D["corrected"]), q(D["has_non_corrected"]),
            q(D["non_corrected"]), q(D["pose_out"]), q(D["corrected_by"]), q(D["point_ref_kf"]), q(D["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    if not download:
        return None, D
    s.synchronize()
    return download_loop(c, D), D


def download_loop(c, D):
    nkf, n = c["nkf"], c["npoints"]
    b = lambda k: D[k].cpu().numpy().tobytes()
    return dict(has_corrected=np.frombuffer(b("has_corrected"), np.uint8)[:nkf], corrected=np.frombuffer(b("corrected"), SIM3D_DTYPE)[:nkf],
                has_non_corrected=np.frombuffer(b("has_non_corrected"), np.uint8)[:nkf], non_corrected=np.frombuffer(b("non_corrected"), SIM3D_DTYPE)[:nkf],
                pose_out=np.frombuffer(b("pose_out"), KF_POSE_DTYPE)[:nkf], points=np.frombuffer(b("pts"), MAP_POINT_DTYPE)[:n],
                corrected_by=np.frombuffer(b("corrected_by"), np.int32)[:n], point_ref_kf=np.frombuffer(b("point_ref_kf"), np.int32)[:n],
                info=np.frombuffer(b("info"), np.int32)[:LR.LC_INFO])


def run_host_map(c, ext):
    nkf, n = c["nkf"], c["npoints"]
    pts = c["points"].copy()
    out = dict(pose_out=_sent(nkf, KF_POSE_DTYPE), kf_updated=_sent(nkf, np.uint8), point_updated=_sent(n, np.uint8), info=_sent(LR.MU_INFO, np.int32))
    q = lambda a: None if a is None else _p(a)
    rc = ext._L.pgorb_global_ba_map_update(
        ext._h, nkf, _p(c["pose"]), _p(c["pose_gba"]), _p(c["kf_done"]), _p(c["parent"]), _p(c["kf_origin"]), q(c["kf_bad"]), n, _p(pts),
        _p(c["pos_gba"]), _p(c["point_done"]), q(c["point_bad"]), _p(c["ref_kf"]), _p(out["pose_out"]), _p(out["kf_updated"]),
        _p(out["point_updated"]), _p(out["info"]))
    out["point_updated"] = out["point_updated"][:n]
    out["points"], out["ret"] = pts, rc
    return out


def map_device_arrays(c):
    import torch
    nkf, n = c["nkf"], c["npoints"]
    up = lambda a: None if a is None else torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()
    sent = lambda nbytes: torch.full((max(nbytes, 1),), SENT, dtype=torch.uint8, device="cuda")
    return dict(pose=up(c["pose"]), gba=up(c["pose_gba"]), kd=up(c["kf_done"]), par=up(c["parent"]), org=up(c["kf_origin"]), kb=up(c["kf_bad"]),
                pts=up(c["points"]), pg=up(c["pos_gba"]), pd=up(c["point_done"]), pb=up(c["point_bad"]), rk=up(c["ref_kf"]),
                pose_out=sent(nkf * KF_POSE_DTYPE.itemsize), kf_updated=sent(nkf), point_updated=sent(n), info=sent(LR.MU_INFO * 4))


def run_device_map(c, ext, stream=None, D=None, download=True):
    import torch
    D = map_device_arrays(c) if D is None else D
    q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        rc = ext._L.pgorb_global_ba_map_update_device(
            ext._h, c["nkf"], q(D["pose"]), q(D["gba"]), q(D["kd"]), q(D["par"]), q(D["org"]), q(D["kb"]), c["npoints"], q(D["pts"]), q(D["pg"]),
            q(D["pd"]), q(D["pb"]), q(D["rk"]), q(D["pose_out"]), q(D["kf_updated"]), q(D["point_updated"]), q(D["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    if not download:
        return None, D
    s.synchronize()
    nkf, n = c["nkf"], c["npoints"]
    b = lambda k: D[k].cpu().numpy().tobytes()
    return dict(pose_out=np.frombuffer(b("pose_out"), KF_POSE_DTYPE)[:nkf], kf_updated=np.frombuffer(b("kf_updated"), np.uint8)[:nkf],
                points=np.frombuffer(b("pts"), MAP_POINT_DTYPE)[:n], point_updated=np.frombuffer(b("point_updated"), np.uint8)[:n],
                info=np.frombuffer(b("info"), np.int32)[:LR.MU_INFO]), D
