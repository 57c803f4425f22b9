"""Cases for tests/test_track_pose.py: the constructed key-frame tables and trajectory records, the predict / commit sequences, the
mTcp list, the seeded random worlds, the float64 anchor with its bound, and the runners of the library's entry points.  A case is
a dict: name, pose [nkf] (KF_POSE_DTYPE), kf_bad, parent, kf_id, tcp [nkf][12], traj [n] (TRAJECTORY_RECORD_DTYPE)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_pose_reference as TR  # noqa: E402
from track_pose_reference import KF_POSE_DTYPE, TRACK_STATE_DTYPE, TRAJECTORY_RECORD_DTYPE  # noqa: E402

f32, f64 = np.float32, np.float64
TRAJ_KEYS = ("quat_wxyz", "translation", "time_usec", "frame_id", "is_lost", "status", "info")
SENT = 0xA5
CAM = (500.0, 510.0, 320.0, 240.0)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def stack(recs, dtype):
    """a 1-d structured array of the given 0-d records"""
    out = np.zeros(len(recs), dtype)
    for i, r in enumerate(recs):
        out[i] = np.asarray(r, dtype).reshape(-1)[0]
    return out


def same(a, b, keys=TRAJ_KEYS):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k in keys)


# ---------------------------------------------------------------- builders
def rot(axis, deg):
    """a float64 rotation about `axis` (Rodrigues)"""
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f64)
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rows(R, t):
    """pose rows [12] in float32 of [R | t]"""
    return np.concatenate([np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3, 1)], 1).reshape(12)


def make_pose(R, t):
    """a KF_POSE_DTYPE record with SetPose's Ow and the camera"""
    p = np.zeros((), KF_POSE_DTYPE)
    p["Tcw"] = rows(R, t)
    p["Ow"] = TR.set_pose_ow(p["Tcw"])
    p["fx"], p["fy"], p["cx"], p["cy"] = CAM
    p["invfx"], p["invfy"] = f32(1) / f32(CAM[0]), f32(1) / f32(CAM[1])
    return p


def record(pose_rows, ref_kf, time, fid, lost=0, has_pose=1):
    r = np.zeros((), TRAJECTORY_RECORD_DTYPE)
    r["pose"], r["ref_kf"], r["frame_time"], r["frame_id"], r["lost"], r["has_pose"] = pose_rows, ref_kf, time, fid, lost, has_pose
    return r


def frozen_tcp(pose, parent, bad):
    """mTcp as SetBadFlag leaves it for every culled key frame with a parent in range, zeros elsewhere"""
    tcp = np.zeros((len(pose), 12), f32)
    for k in range(len(pose)):
        if bad[k] and 0 <= parent[k] < len(pose):
            tcp[k] = TR.mul44(TR.mat44(pose[k]["Tcw"]), TR.pose_inverse(pose[parent[k]]["Tcw"], pose[parent[k]]["Ow"]))[:3].reshape(12)
    return tcp


def case(name, poses, bad, parent, ids, traj, tcp=None):
    pose = np.array(poses, KF_POSE_DTYPE).reshape(-1)
    bad, parent = np.array(bad, np.uint8), np.array(parent, np.int32)
    return dict(name=name, pose=pose, kf_bad=bad, parent=parent, kf_id=np.array(ids, np.uint64),
                tcp=frozen_tcp(pose, parent, bad) if tcp is None else np.array(tcp, f32).reshape(-1, 12),
                traj=np.array(traj, TRAJECTORY_RECORD_DTYPE).reshape(-1))


I3, Z3 = np.eye(3), np.zeros(3)
PERM = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], f64)             # 120 degrees about (1, 1, 1): trace exactly 0


def trajectory_cases():
    out = []
    ident = make_pose(I3, Z3)
    # 1. one live key frame, one record, identity everywhere
    out.append(case("identity", [ident], [0], [-1], [0], [record(rows(I3, Z3), 0, 1.5, 7)]))
    # 2. the other three branches of Quaterniond(R) and the t > 0 boundary
    half = [record(rows(np.diag(d), [0.5, -0.25, 2.0]), 0, 0.1 * i, i) for i, d in enumerate(([1., -1, -1], [-1., 1, -1], [-1., -1, 1]))]
    out.append(case("half_turns", [ident], [0], [-1], [0], half + [record(rows(PERM, [1.0, 2.0, 3.0]), 0, 0.3, 3)]))
    # 3. three culled key frames in a chain under a live one, and a culled child of the origin; a record at each depth
    P = [make_pose(rot([1, 2, 3], 10.0 * k + 5), [0.3 * k, -0.2 * k + 0.1, 0.05 * k * k]) for k in range(6)]
    rel = lambda i: rows(rot([3, -1, 2], 7.0 * i + 1), [0.01 * i, 0.02, -0.03 * i])
    out.append(case("chain", P, [0, 0, 1, 1, 1, 1], [-1, 0, 1, 2, 3, 0], [0, 1, 2, 3, 4, 5],
                    [record(rel(i), k, 1.0 + i / 30.0, 100 + i) for i, k in enumerate((1, 2, 3, 4, 5, 0))]))
    # 4. the origin is not index 0; a bad key frame carries the smallest mnId; ids above 2^32 (truncated to 32 bits, key frame 0 wins)
    out.append(case("origin", P[:4], [0, 1, 0, 0], [2, 2, -1, 2], [(1 << 33) + 5, 3, (1 << 32) + 7, 1 << 40],
                    [record(rel(i), k, 2.0 + i, i) for i, k in enumerate((0, 1, 2, 3))]))
    # 5. poses holding -0.0 and translations that cancel to zero (tests/test_track_pose.py writes the expectations out)
    nz = f32(-0.0)
    half_z = np.array([[-1, nz, nz], [nz, -1, nz], [0, 0, 1]], f32)   # 180 degrees about z with negative zeros in its first two rows
    tcp = np.zeros((2, 12), f32)
    tcp[1] = rows(half_z, [-1.0, -2.0, 0.0])
    diag45 = rot([0, 0, 1], 45.0)
    out.append(case("signed_zeros", [ident, ident], [0, 1], [-1, 0], [0, 1],
                    [record(rows(half_z, [nz, nz, nz]), 1, 0.0, 0),                      # through eye*mTcp
                     record(rows(I3, Z3), 1, 0.0, 1),
                     record(rows(half_z, [nz, nz, nz]), 0, 0.0, 2),                      # no culled key frame on the way
                     record(rows(diag45, [1.0, -1.0, 0.0]), 0, 0.0, 3)], tcp=tcp))       # R' t cancels in its first component
    # ... and a product whose first three terms are all -0 while the fourth, tx * 0, is +0: the sum is +0 only if it is formed
    pk = np.zeros((), KF_POSE_DTYPE)
    pk["Tcw"] = rows(np.array([[1, 0, nz], [0, -1, 0], [nz, nz, -1]], f32), [0.0, -2.0, 1.0])
    pk["Ow"] = TR.set_pose_ow(pk["Tcw"])
    out.append(case("signed_zeros_fourth_term", [pk], [0], [-1], [0],
                    [record(rows(np.array([[1, nz, nz], [0, -1, nz], [0, nz, -1]], f32), [2.0, 0.0, 0.0]), 0, 0.0, 0)]))
    # 6. lost records first, last and interleaved; a lost record without a pose and with a reference that names nothing
    lostcase = []
    for i, (lost, hp, k) in enumerate(((1, 1, 0), (0, 1, 1), (1, 0, -5), (0, 1, 0), (1, 1, 7), (0, 1, 1), (1, 0, 0))):
        lostcase.append(record(rel(i) if hp else np.full(12, np.nan, f32), k, 3.0 + i, 10 * i, lost=lost, has_pose=hp))
    out.append(case("lost", P[:2], [0, 0], [-1, 0], [5, 6], lostcase))
    # 7. the issue's times, and three whose product with 1e6 has a fraction above one half: truncation, rounding and flooring part there
    out.append(case("times", [ident], [0], [-1], [0],
                    [record(rows(I3, Z3), 0, t, i) for i, t in enumerate((0.29, 0.1, 1e9 + 0.999999, -0.29, 0.2999999, 2.0000007, -0.2999999, -1e-7,
                                                                         0.0))]))
    # 8. broken tables: key frame 1 is bad without a parent, 2 and 3 are a two-cycle of bad key frames
    out.append(case("broken", [ident, P[1], P[2], P[3]], [0, 1, 1, 1], [-1, -1, 3, 2], [0, 1, 2, 3],
                    [record(rel(0), 0, 0.0, 0), record(rel(1), 1, 0.1, 1), record(rel(2), 0, 0.2, 2), record(rel(3), 2, 0.3, 3),
                     record(rel(4), 4, 0.4, 4), record(rel(5), 0, 0.5, 5, has_pose=0), record(rel(6), 0, 0.6, 6), record(rel(7), -1, 0.7, 7)],
                    tcp=np.stack([np.zeros(12, f32), rows(rot([1, 0, 0], 3), [0.1, 0, 0]), rows(rot([0, 1, 0], 3), [0, 0.1, 0]), rows(rot([0, 0, 1], 3), [0, 0, 0.1])])))
    return out


BROKEN_EXPECTED = [0, TR.BROKEN, 0, TR.BROKEN, TR.BROKEN, TR.BROKEN, 0, TR.BROKEN]


# ---------------------------------------------------------------- random worlds
WORLD_RECORDS, WORLD_KFS = (1, 63, 64, 65, 257, 4099), (1, 2, 17, 300)


def chain_f64(c, i):
    """(the float64 product eye * mTcp ... * Tcw[k], k, depth) of record i's walk, or None when it breaks"""
    k, d, nkf = int(c["traj"][i]["ref_kf"]), 0, len(c["pose"])
    T = np.eye(4)
    while True:
        if not 0 <= k < nkf or d >= nkf:
            return None
        if not c["kf_bad"][k]:
            return T @ TR.mat44(c["pose"][k]["Tcw"]).astype(f64), k, d
        T = T @ TR.mat44(c["tcp"][k]).astype(f64)
        k, d = int(c["parent"][k]), d + 1


def random_world(seed, n, nkf, culled=0.4, exact=False):
    """nkf key frames in a random spanning tree with up to `culled` of them bad in chains, ids in random order (some above 2^32),
    n records: one in ten lost, one in seven steered so that the final rotation is a half turn about an axis"""
    rng = np.random.default_rng([seed, n, nkf])
    pose = np.array([make_pose(rot(rng.normal(size=3), rng.uniform(-180, 180)), rng.normal(0, 2, 3)) for _ in range(nkf)], KF_POSE_DTYPE)
    parent = np.array([-1] + [k - 1 if rng.random() < 0.6 else int(rng.integers(0, k)) for k in range(1, nkf)], np.int32)
    bad = np.zeros(nkf, np.uint8)
    if nkf > 1:
        nb = int(culled * nkf) if exact else int(rng.integers(0, int(culled * nkf) + 1))
        start = int(rng.integers(1, nkf))
        run = np.arange(start, min(start + max(nb // 2, 1), nkf))                  # a run of consecutive indices: chains
        bad[run[:nb]] = 1
        rest = nb - int(bad.sum())
        if rest > 0:
            bad[rng.choice(np.nonzero(bad[1:] == 0)[0] + 1, rest, replace=False)] = 1
    ids = rng.permutation(nkf).astype(np.uint64) * np.uint64(3) + np.uint64(1)
    ids[rng.random(nkf) < 0.3] += np.uint64(1 << 32)
    c = case("world_%d_%d_%d" % (seed, n, nkf), pose, bad, parent, ids, [])
    o = TR.origin_of(c["kf_bad"], c["kf_id"])
    Two = np.linalg.inv(TR.mat44(pose[o]["Tcw"]).astype(f64))
    traj = np.zeros(n, TRAJECTORY_RECORD_DTYPE)
    for i in range(n):
        traj[i] = record(rows(rot(rng.normal(size=3), rng.uniform(-30, 30)), rng.normal(0, 0.1, 3)), int(rng.integers(0, nkf)), 10.0 + i / 30.0, i)
    c["traj"] = traj
    for i in range(n):
        u = rng.random()
        if u < 0.1:
            traj[i]["lost"], traj[i]["has_pose"] = 1, rng.random() < 0.7
        elif u < 0.25:
            ch = chain_f64(c, i)
            if ch is not None:                                                      # rel = target * (chain * Two)^-1
                target = np.eye(4)
                target[:3, :3] = rot(np.eye(3)[int(rng.integers(0, 3))], 180.0) @ rot(rng.normal(size=3), rng.uniform(-2, 2))
                M = target @ np.linalg.inv(ch[0] @ Two)
                traj[i]["pose"] = rows(M[:3, :3], M[:3, 3])
    return c


def large_world():
    """108 000 records (an hour at 30 frames a second) over 2 000 key frames, 30 % of them culled"""
    return random_world(1, 108000, 2000, culled=0.3, exact=True)


# ---------------------------------------------------------------- the float64 anchor
U32 = 2.0 ** -24


def quat_from_K(R):
    """the unit quaternion (w, x, y, z) of a rotation as the top eigenvector of Bar-Itzhack's symmetric 4 x 4 K matrix"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0],
                  [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]], f64) / 3.0
    w, v = np.linalg.eigh(K, UPLO="L")
    q = v[:, np.argmax(w)]
    return np.array([q[3], q[0], q[1], q[2]])


def anchor(c, i):
    """Record i in plain float64 algebra with its error bound against the float32 restatement.  Returns (quat, translation,
    bound_quat, bound_translation) or None for a lost or broken record.

    The bound is a running first-order error analysis of the float32 chain.  A float32 product C = A*B of 4 x 4 matrices with
    four terms per element has |C - AB| <= 4u |A||B| (u = 2^-24: three additions and a product per term, Higham's gamma_4), and
    errors E_A, E_B already in the operands add E_A|B| + |A|E_B + E_A E_B.  The chain has depth + 3 products (depth identity-side
    products, Trw*Tcw, *Two, rel*), each taken in turn.  Two itself differs from the true inverse because the stored Ow is a float32
    -R't (4u |R|'|t|) and because R' is the inverse of R only up to d_o = max|RR' - I| (taken four times, entrywise, with the
    translation it multiplies).  The translation -R't of the result adds E|t| + |R|E_t + 4u |R|'|t|.  The two quaternion methods
    are each Lipschitz in the matrix entries with a constant below 4 (Eigen's: the pivot is 0.5 sqrt(1 + s) with s >= 0, so 0.75 eps
    on the pivot and 2.5 eps on the others; the eigenvector's: ||dK|| <= 4 eps over a spectral gap of 4/3), and they see a matrix
    that is orthogonal only up to d = max|RR' - I| of the float64 result, so they differ by at most 4 eps + 8 d."""
    r = c["traj"][i]
    if r["lost"] or not r["has_pose"]:
        return None
    ch = chain_f64(c, i)
    if ch is None:
        return None
    _, k, depth = ch
    o = TR.origin_of(c["kf_bad"], c["kf_id"])
    A = lambda x: np.abs(x)
    def mul(X, EX, Y, EY):
        return X @ Y, EX @ A(Y) + A(X) @ EY + EX @ EY + 4 * U32 * (A(X) @ A(Y))
    T, E = np.eye(4), np.zeros((4, 4))
    kk = int(r["ref_kf"])
    for _ in range(depth):
        T, E = mul(T, E, TR.mat44(c["tcp"][kk]).astype(f64), np.zeros((4, 4)))
        kk = int(c["parent"][kk])
    T, E = mul(T, E, TR.mat44(c["pose"][k]["Tcw"]).astype(f64), np.zeros((4, 4)))
    To = TR.mat44(c["pose"][o]["Tcw"]).astype(f64)
    Ro, to = To[:3, :3], To[:3, 3]
    d_o = np.abs(Ro @ Ro.T - np.eye(3)).max()
    ETwo = np.zeros((4, 4))
    ETwo[:3, :3] = 4 * d_o
    ETwo[:3, 3] = 4 * U32 * (A(Ro).T @ A(to)) + 4 * d_o * A(to).sum()
    T, E = mul(T, E, np.linalg.inv(To), ETwo)
    T, E = mul(TR.mat44(r["pose"]).astype(f64), np.zeros((4, 4)), T, E)
    R, t = T[:3, :3].T, T[:3, 3]
    trans = -R @ t
    bt = E[:3, :3].T @ A(t) + A(R) @ E[:3, 3] + 4 * U32 * (A(R) @ A(t)) + U32 * A(trans)
    d = np.abs(R @ R.T - np.eye(3)).max()
    bq = 4 * E[:3, :3].max() + 8 * d + 1e-15
    return quat_from_K(R), trans, bq, bt


# ---------------------------------------------------------------- predict / commit sequences
CAP = 5


def track_sequences():
    """Two trackers over six frames and a capacity of five records.  Per frame: the key-frame table as it stands, and per tracker
    (mode, the frame's final pose, bOK, mpReferenceKF, time, id).  Tracker 0: reference-KF mode twice, the motion model, a lost
    frame, the motion model again with the velocity the lost frame left, a reference change, and the sixth commit finds the array
    full.  Tracker 1 is lost earlier and changes its reference later.  The key frames move after frame 2 (local mapping), so
    UpdateLastFrame has something to do."""
    kf_a = np.array([make_pose(rot([1, 1, 0], 4.0 * k), [0.2 * k, 0.0, 0.1 * k]) for k in range(4)], KF_POSE_DTYPE)
    kf_b = np.array([make_pose(rot([1, 1, 0.1], 4.0 * k + 0.3), [0.2 * k + 0.01, -0.01, 0.1 * k]) for k in range(4)], KF_POSE_DTYPE)
    final = lambda t, f: make_pose(rot([0.2, 1, 0.1 * t], 3.0 * f + t), [0.05 * f + 0.3 * t, 0.01 * f, 0.11 * f])
    M, K = TR.MOTION_MODEL, TR.REFERENCE_KF
    modes = ((K, M), (K, K), (M, M), (M, M), (M, K), (M, M))
    oks = ((1, 1), (1, 1), (1, 0), (0, 1), (1, 1), (1, 1))
    refs = ((0, 1), (0, 1), (0, 1), (0, 1), (2, 1), (2, 3))
    frames = []
    for f in range(6):
        frames.append(dict(kf=kf_a if f < 3 else kf_b,
                           trackers=[dict(mode=modes[f][t], pose=final(t, f), ok=oks[f][t], ref_kf=refs[f][t], time=100.0 + f / 30.0 + t, id=1000 * t + f)
                                     for t in range(2)]))
    cam = make_pose(I3, Z3)
    state = np.zeros(2, TRACK_STATE_DTYPE)
    for t in range(2):
        state[t]["last_ref_kf"] = -1
        for k in ("fx", "fy", "cx", "cy", "invfx", "invfy"):
            state[t]["last"][k] = cam[k]
    return state, frames


def run_sequences_reference(rules=TR.REFERENCE, literal=False):
    """per frame: (predicted poses [2], predict status [2], states after predict, commit status [2], states after commit, records
    [2][CAP] with the untouched entries SENT, counts [2])"""
    state, frames = track_sequences()
    fill = np.frombuffer(bytes([SENT]) * (CAP * TRAJECTORY_RECORD_DTYPE.itemsize), TRAJECTORY_RECORD_DTYPE)
    trk = [TR.Tracker(state[t], cap=CAP) for t in range(2)]
    out = []
    for fr in frames:
        pred, ps, cs = np.zeros(2, KF_POSE_DTYPE), np.zeros(2, np.int32), np.zeros(2, np.int32)
        for t in range(2):
            pred[t], ps[t] = TR.predict(trk[t], fr["trackers"][t]["mode"], fr["kf"], rules, literal)
        mid = stack([trk[t].state() for t in range(2)], TRACK_STATE_DTYPE)
        for t in range(2):
            x = fr["trackers"][t]
            cs[t] = TR.commit(trk[t], x["pose"], x["ok"], x["ref_kf"], x["time"], x["id"], fr["kf"], CAP, rules, literal)
        out.append(dict(pred=pred, pred_status=ps, state_mid=mid, commit_status=cs, state=stack([trk[t].state() for t in range(2)], TRACK_STATE_DTYPE),
                        traj=np.stack([trk[t].records(CAP, fill) for t in range(2)]), count=np.array([len(trk[t].trajectory) for t in range(2)], np.int32)))
    return out


SEQ_KEYS = ("pred", "pred_status", "state_mid", "commit_status", "state", "traj", "count")


# ---------------------------------------------------------------- the mTcp list
def tcp_case():
    """six key frames; a list of six members -- two culled with a parent, one kept, one WAS_BAD, one culled whose parent is -1,
    one culled that names no key frame -- and two stale rows behind the list's length that say CULLED"""
    pose = np.array([make_pose(rot([1, 2, 3], 9.0 * k + 2), [0.3 * k, 0.1, -0.2 * k]) for k in range(6)], KF_POSE_DTYPE)
    parent = np.array([-1, 0, 1, 1, 2, 0], np.int32)
    rec = np.array([[2, 40, 39, 1], [3, 40, 10, 0], [4, 17, 17, 1], [5, 12, 12, 4], [0, 9, 9, 1], [9, 1, 1, 1], [1, 5, 5, 1], [3, 5, 5, 1]], np.int32)
    return dict(pose=pose, parent=parent, record=rec, nlist=6, tcp=np.frombuffer(bytes([SENT]) * (6 * 48), f32).reshape(6, 12).copy())


# ---------------------------------------------------------------- the library
def _up(a):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def _sent(nbytes):
    import torch
    return torch.full((max(nbytes, 1),), SENT, dtype=torch.uint8, device="cuda")


def _q(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def table_device_arrays(c):
    return dict(pose=_up(c["pose"]), bad=_up(c["kf_bad"]), par=_up(c["parent"]), ids=_up(c["kf_id"]), tcp=_up(c["tcp"]))


def run_get_trajectory_device(c, ext, stream=None, n=None, count=None, D=None):
    """pgorb_get_trajectory_device on resident arrays whose outputs start as SENT; returns what was downloaded, cut to the count"""
    import torch
    D = table_device_arrays(c) if D is None else D
    nrec = len(c["traj"]) if n is None else n
    traj = _up(c["traj"]) if len(c["traj"]) else _sent(8)
    O = dict(quat_wxyz=_sent(nrec * 32), translation=_sent(nrec * 24), time_usec=_sent(nrec * 8), frame_id=_sent(nrec * 8), is_lost=_sent(nrec),
             status=_sent(nrec * 4), info=_sent(TR.TRAJ_INFO * 4))
    cnt = None if count is None else _up(np.array([count], np.int32))
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()                                        # the arrays were filled on the current stream
    with torch.cuda.stream(s):
        rc = ext._L.pgorb_get_trajectory_device(ext._h, len(c["pose"]), _q(D["pose"]), _q(D["bad"]), _q(D["par"]), _q(D["ids"]), _q(D["tcp"]), nrec,
                                                _q(traj), _q(cnt), _q(O["quat_wxyz"]), _q(O["translation"]), _q(O["time_usec"]), _q(O["frame_id"]),
                                                _q(O["is_lost"]), _q(O["status"]), _q(O["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    s.synchronize()
    return download_trajectory(O, nrec)


def download_trajectory(O, nrec):
    b = lambda k: O[k].cpu().numpy().tobytes()
    return dict(quat_wxyz=np.frombuffer(b("quat_wxyz"), f64)[:nrec * 4].reshape(nrec, 4), translation=np.frombuffer(b("translation"), f64)[:nrec * 3].reshape(nrec, 3),
                time_usec=np.frombuffer(b("time_usec"), np.int64)[:nrec], frame_id=np.frombuffer(b("frame_id"), np.int64)[:nrec],
                is_lost=np.frombuffer(b("is_lost"), np.uint8)[:nrec], status=np.frombuffer(b("status"), np.int32)[:nrec],
                info=np.frombuffer(b("info"), np.int32)[:TR.TRAJ_INFO])


def run_get_trajectory_host(c, ext):
    """pgorb_get_trajectory itself; returns (return value, outputs)"""
    n = len(c["traj"])
    n1 = max(n, 1)
    O = dict(quat_wxyz=np.zeros((n1, 4), f64), translation=np.zeros((n1, 3), f64), time_usec=np.zeros(n1, np.int64), frame_id=np.zeros(n1, np.int64),
             is_lost=np.zeros(n1, np.uint8), status=np.zeros(n1, np.int32), info=np.zeros(TR.TRAJ_INFO, np.int32))
    traj = c["traj"] if n else np.zeros(1, TRAJECTORY_RECORD_DTYPE)
    rc = ext._L.pgorb_get_trajectory(ext._h, len(c["pose"]), _p(c["pose"]), _p(c["kf_bad"]), _p(c["parent"]), _p(c["kf_id"]), _p(c["tcp"]), n, _p(traj),
                                     _p(O["quat_wxyz"]), _p(O["translation"]), _p(O["time_usec"]), _p(O["frame_id"]), _p(O["is_lost"]), _p(O["status"]),
                                     _p(O["info"]))
    return rc, {k: (v if k == "info" else v[:n]) for k, v in O.items()}


def padded(e, nrec):
    """the reference's outputs as the device leaves arrays of nrec entries that started as SENT"""
    out = {}
    for k, dt, w in (("quat_wxyz", f64, 4), ("translation", f64, 3), ("time_usec", np.int64, 1), ("frame_id", np.int64, 1), ("is_lost", np.uint8, 1),
                     ("status", np.int32, 1)):
        a = np.frombuffer(bytes([SENT]) * (nrec * w * np.dtype(dt).itemsize), dt).copy().reshape((nrec, w) if w > 1 else (nrec,))
        if k in e:
            a[:len(e[k])] = e[k]
        out[k] = a
    out["info"] = e["info"]
    return out


def run_sequences_device(ext, stream=None):
    """the six frames on resident arrays, both trackers per call; what run_sequences_reference returns"""
    import torch
    state, frames = track_sequences()
    s = stream if stream is not None else torch.cuda.current_stream()
    S, T, N = _up(state), _sent(2 * CAP * TRAJECTORY_RECORD_DTYPE.itemsize), _up(np.zeros(2, np.int32))
    down = lambda t, dt: np.frombuffer(t.cpu().numpy().tobytes(), dt).copy()
    out = []
    torch.cuda.synchronize()                                        # the arrays were filled on the current stream
    with torch.cuda.stream(s):
        for fr in frames:
            x = fr["trackers"]
            kf = _up(fr["kf"])
            modes = _up(np.array([v["mode"] for v in x], np.int32))
            pred, ps, cs = _sent(2 * KF_POSE_DTYPE.itemsize), _sent(8), _sent(8)
            rc = ext._L.pgorb_track_predict_batch_device(ext._h, 2, 0, _q(modes), _q(S), _q(T), CAP, _q(N), len(fr["kf"]), _q(kf), _q(pred), _q(ps),
                                                         C.c_void_p(s.cuda_stream))
            assert rc == 0, rc
            s.synchronize()
            mid = down(S, TRACK_STATE_DTYPE)
            pose, ok, ref = _up(stack([v["pose"] for v in x], KF_POSE_DTYPE)), _up(np.array([v["ok"] for v in x], np.uint8)), \
                _up(np.array([v["ref_kf"] for v in x], np.int32))
            tm, ids = _up(np.array([v["time"] for v in x], f64)), _up(np.array([v["id"] for v in x], np.int64))
            rc = ext._L.pgorb_track_commit_batch_device(ext._h, 2, _q(S), _q(pose), _q(ok), _q(ref), _q(tm), _q(ids), len(fr["kf"]), _q(kf), _q(T), CAP,
                                                        _q(N), _q(cs), C.c_void_p(s.cuda_stream))
            assert rc == 0, rc
            s.synchronize()
            out.append(dict(pred=down(pred, KF_POSE_DTYPE), pred_status=down(ps, np.int32), state_mid=mid, commit_status=down(cs, np.int32),
                            state=down(S, TRACK_STATE_DTYPE), traj=down(T, TRAJECTORY_RECORD_DTYPE).reshape(2, CAP), count=down(N, np.int32)))
    return out


def run_sequences_host(ext):
    """the same through the single calls, a tracker at a time"""
    state, frames = track_sequences()
    st = [state[t:t + 1].copy() for t in range(2)]
    traj = [np.frombuffer(bytes([SENT]) * (CAP * TRAJECTORY_RECORD_DTYPE.itemsize), TRAJECTORY_RECORD_DTYPE).copy() for _ in range(2)]
    cnt = [np.zeros(1, np.int32) for _ in range(2)]
    out = []
    for fr in frames:
        pred, ps, cs = np.zeros(2, KF_POSE_DTYPE), np.zeros(2, np.int32), np.zeros(2, np.int32)
        for t in range(2):
            x = fr["trackers"][t]
            last = traj[t][cnt[t][0] - 1:cnt[t][0]] if cnt[t][0] else None
            ps[t] = ext._L.pgorb_track_predict(ext._h, x["mode"], _p(st[t]), None if last is None else _p(np.ascontiguousarray(last)), len(fr["kf"]),
                                               _p(fr["kf"]), _p(pred[t:t + 1]))
        mid = np.concatenate(st)
        for t in range(2):
            x = fr["trackers"][t]
            pose = np.array(x["pose"])
            cs[t] = ext._L.pgorb_track_commit(ext._h, _p(st[t]), _p(pose), int(x["ok"]), int(x["ref_kf"]), float(x["time"]), int(x["id"]),
                                              len(fr["kf"]), _p(fr["kf"]), _p(traj[t]), CAP, _p(cnt[t]))
        out.append(dict(pred=pred, pred_status=ps, state_mid=mid, commit_status=cs, state=np.concatenate(st), traj=np.stack(traj).copy(),
                        count=np.array([cnt[0][0], cnt[1][0]], np.int32)))
    return out


def run_tcp_device(c, ext, stream=None, limit=False):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    D = dict(pose=_up(c["pose"]), par=_up(c["parent"]), rec=_up(c["record"]), ci=_up(np.array([TR.CULL_LIMIT if limit else 0, c["nlist"], 0, 0], np.int32)),
             tcp=_up(c["tcp"]), info=_sent(TR.TCP_INFO * 4))
    torch.cuda.synchronize()                                        # the arrays were filled on the current stream
    with torch.cuda.stream(s):
        rc = ext._L.pgorb_keyframe_tcp_device(ext._h, len(c["pose"]), _q(D["pose"]), _q(D["par"]), len(c["record"]), _q(D["rec"]), _q(D["ci"]), _q(D["tcp"]),
                                              _q(D["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    s.synchronize()
    return np.frombuffer(D["tcp"].cpu().numpy().tobytes(), f32).reshape(-1, 12), np.frombuffer(D["info"].cpu().numpy().tobytes(), np.int32)[:TR.TCP_INFO]


def run_tcp_host(c, ext):
    tcp, info = c["tcp"].copy(), np.zeros(TR.TCP_INFO, np.int32)
    rec = np.ascontiguousarray(c["record"][:c["nlist"]])
    rc = ext._L.pgorb_keyframe_tcp(ext._h, len(c["pose"]), _p(c["pose"]), _p(c["parent"]), len(rec), _p(rec), _p(tcp), _p(info))
    return rc, tcp, info
