"""A numpy restatement of the tracking thread's pose bookkeeping and of System::GetTrajectory, written from the reference's source
lines (thirdparty/orb-slam2), not from csrc/track_pose.hip:

  predict          Tracking::UpdateLastFrame, the monocular return (src/Tracking.cc:792-798), then :866
                   mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw), or :764 SetPose(mLastFrame.mTcw)
  commit           the end of Tracking::Track: the motion model (:432-440), mLastFrame = Frame(mCurrentFrame) (:493), the
                   RelativeFramePoseData record (:497-506)
  keyframe_tcp     KeyFrame::SetBadFlag's mTcp = Tcw*mpParent->GetPoseInverse() (src/KeyFrame.cc:641)
  get_trajectory   System::GetTrajectory (src/System.cc:371-412)

The readings of cv::Mat arithmetic are DESIGN.md section 4's: a 4 x 4 CV_32F product is gemm's small-matrix path, the four terms in
index order in float, every term formed; SetPose's Ow = -Rcw.t()*tcw and GetTrajectory's -rotation_mat*t are that path with alpha =
-1 applied in double; Converter::toEigenQuaternion is Eigen's Quaterniond(Matrix3d) on the floats widened to double, math.sqrt for
the root.  Two forms: the default one uses float32 array operations one at a time; `literal=True` runs explicit loops with the
four terms written out.  tests/test_track_pose.py compares them on every case.

Where the reference would dereference NULL, spin or assert (a parent of -1 under a bad key frame, an index out of range, a cycle of
bad key frames, a live record without a pose) the record is marked BROKEN and gives seven zeros -- the contract of include/pgorb.h.
`rules` (a Rules) switches one reading at a time; MUTANTS names them.  `hits` counts branches."""
import math
import os
import sys
from dataclasses import dataclass, replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pilotguru_amd._lib import KF_POSE_DTYPE, TRACK_STATE_DTYPE, TRAJECTORY_RECORD_DTYPE  # noqa: E402

f32, f64 = np.float32, np.float64
MOTION_MODEL, REFERENCE_KF = 0, 1                                   # PGORB_TRACK_* (include/pgorb.h)
NO_LAST, NO_VELOCITY, BAD_INDEX, FULL = 1, 2, 4, 8
BROKEN, BAD_TIME, NO_ORIGIN, TRAJ_INFO, TCP_INFO = 1, 2, 4, 4, 4
CULLED, CULL_LIMIT = 1, 32                                          # PGORB_CULL_KF_CULLED, PGORB_CULL_LIMIT
INT64_MIN = -2 ** 63


@dataclass(frozen=True)
class Rules:
    grouping: str = "left"            # Trw*pKF->GetPose()*Two and mRelativeFramePose*Trw, left to right (:402-404) | "right"
    identity_product: bool = True     # Trw = eye*mTcp is formed (:394, :398) | False: Trw = mTcp
    fourth_term: bool = True          # the fourth term of a product is formed although its operand is the constant 0 | False
    origin: str = "smallest_live_id"  # vpKFs[0] after sort(lId) over the map's key frames (:374-379) | "index0"
    alpha: str = "double"             # -rotation_mat*t: gemm with alpha = -1 applied to the float sum in double | "float": the matrix
                                      # negated in float first
    quat_of: str = "transposed"       # rotation_mat = the block's .t() (:405) | "block"
    time: str = "truncate"            # static_cast<int64>(mFrameTime*1e6) (:386) | "round"
    lost_velocity: str = "keep"       # mVelocity is touched only if(bOK) (:429-440) | "clear"


REFERENCE = Rules()
MUTANTS = {
    "right_to_left": replace(REFERENCE, grouping="right"),
    "identity_skipped": replace(REFERENCE, identity_product=False),
    "fourth_term_dropped": replace(REFERENCE, fourth_term=False),
    "origin_index0": replace(REFERENCE, origin="index0"),
    "alpha_in_float": replace(REFERENCE, alpha="float"),
    "quat_untransposed": replace(REFERENCE, quat_of="block"),
    "time_rounded": replace(REFERENCE, time="round"),
    "velocity_cleared_when_lost": replace(REFERENCE, lost_velocity="clear"),
}


def _hit(hits, k):
    if hits is not None:
        hits[k] = hits.get(k, 0) + 1


# ---------------------------------------------------------------- cv::Mat
def mat44(rows):
    """the 4 x 4 CV_32F matrix of pose rows [12]"""
    T = np.zeros((4, 4), f32)
    T[:3, :] = np.asarray(rows, f32).reshape(3, 4)
    T[3, 3] = 1
    return T


def eye44():
    return np.eye(4, dtype=f32)


def pose_inverse(Tcw, Ow):
    """GetPoseInverse(): Twc = [Rcw' | Ow], Ow as stored (KeyFrame.cc:61-93); also Track()'s LastTwc (:434-436)"""
    W = eye44()
    W[:3, :3] = mat44(Tcw)[:3, :3].T
    W[:3, 3] = np.asarray(Ow, f32)
    return W


def mul44(A, B, rules=REFERENCE, literal=False):
    """cv::Mat A*B of two 4 x 4 CV_32F matrices whose fourth rows are (0, 0, 0, 1)"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    with np.errstate(all="ignore"):
        if literal:
            Cm = np.zeros((4, 4), f32)
            for r in range(4):
                for c in range(4):
                    s = f32(0)
                    for k in range(4):
                        if k == 3 and not rules.fourth_term and B[3, c] == 0:
                            continue                                 # the mutant: "times the constant 0" optimised away
                        t = f32(A[r, k] * B[k, c])
                        s = t if k == 0 else f32(s + t)
                    Cm[r, c] = s
            return Cm
        s = A[:, [0]] * B[[0], :]
        s = s + A[:, [1]] * B[[1], :]
        s = s + A[:, [2]] * B[[2], :]
        t = A[:, [3]] * B[[3], :]
        if rules.fourth_term:
            return s + t
        return np.where(B[[3], :] == 0, s, s + t).astype(f32)


def set_pose_ow(Tcw, rules=REFERENCE, literal=False):
    """-Rcw.t()*tcw of pose rows [12] (Frame::SetPose / KeyFrame::SetPose, and System.cc:407): float [3]"""
    T = np.asarray(Tcw, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        if rules.alpha == "float":
            N = -T[:, :3]
            if literal:
                return np.array([f32(f32(f32(N[0, i] * T[0, 3]) + f32(N[1, i] * T[1, 3])) + f32(N[2, i] * T[2, 3])) for i in range(3)], f32)
            return (N[0, :] * T[0, 3] + N[1, :] * T[1, 3]) + N[2, :] * T[2, 3]
        if literal:
            return np.array([f32(f64(f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3]))) * f64(-1.0))
                             for i in range(3)], f32)
        s = (T[0, :3] * T[0, 3] + T[1, :3] * T[1, 3]) + T[2, :3] * T[2, 3]
        return (s.astype(f64) * f64(-1.0)).astype(f32)


def quat_branch(R):
    """the branch Eigen's Quaterniond(Matrix3d) takes: 'trace', 'x', 'y' or 'z'"""
    if (R[0][0] + R[1][1]) + R[2][2] > 0:
        return "trace"
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    return "xyz"[i]


def quat_wxyz(R):
    """Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl) of a 3 x 3 double matrix"""
    m = [[float(R[r][c]) for c in range(3)] for r in range(3)]
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]                                        # w, x, y, z
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k][j] - m[j][k]) * t
        q[1 + j] = (m[j][i] + m[i][j]) * t
        q[1 + k] = (m[k][i] + m[i][k]) * t
    return np.array(q, f64)


def time_usec(t, rules=REFERENCE):
    """static_cast<int64>(mFrameTime*1e6): (value, in range)"""
    with np.errstate(all="ignore"):
        us = float(f64(t) * f64(1e6))
    if not (math.isfinite(us) and -2.0 ** 63 <= us < 2.0 ** 63):
        return INT64_MIN, False                                     # cvttsd2si's answer
    return (int(round(us)) if rules.time == "round" else int(us)), True


# ---------------------------------------------------------------- the tracker
class Tracker:
    """the pose members of Tracking: mLastFrame (mTcw, mOw, the camera, mpReferenceKF), mVelocity, mlTrajectory"""

    def __init__(self, state=None, trajectory=(), cap=None):
        s = np.zeros((), TRACK_STATE_DTYPE) if state is None else np.array(state, TRACK_STATE_DTYPE).reshape(())
        self.last = np.array(s["last"])                             # the whole record: its bytes travel
        self.has_last = bool(s["has_last"])
        self.velocity = np.array(s["velocity"], f32)
        self.has_velocity = bool(s["has_velocity"])
        self.last_ref = int(s["last_ref_kf"])
        self.trajectory = [np.array(r) for r in np.asarray(trajectory, TRAJECTORY_RECORD_DTYPE).reshape(-1)] if len(trajectory) else []
        self.cap = cap

    def state(self):
        s = np.zeros((), TRACK_STATE_DTYPE)
        s["last"], s["has_last"], s["velocity"], s["has_velocity"], s["last_ref_kf"] = self.last, self.has_last, self.velocity, self.has_velocity, \
            self.last_ref
        return s

    def records(self, cap=None, fill=None):
        """the record array of capacity `cap`: entries past the count keep `fill`'s bytes"""
        cap = len(self.trajectory) if cap is None else cap
        out = np.zeros(cap, TRAJECTORY_RECORD_DTYPE) if fill is None else np.array(fill, TRAJECTORY_RECORD_DTYPE).reshape(cap)
        for i, r in enumerate(self.trajectory):
            out[i] = r
        return out


def predict(trk, mode, kf_pose, rules=REFERENCE, literal=False):
    """(pose the first search starts from, status); trk.last is updated by UpdateLastFrame"""
    nkf = len(kf_pose)
    status = 0 if trk.has_last else NO_LAST
    if mode == MOTION_MODEL:
        if not trk.has_velocity:
            status |= NO_VELOCITY
        if not 0 <= trk.last_ref < nkf or not trk.trajectory or (trk.cap is not None and len(trk.trajectory) > trk.cap) or \
                not trk.trajectory[-1]["has_pose"]:
            status |= BAD_INDEX
    elif mode != REFERENCE_KF:
        status |= BAD_INDEX
    if status:
        return np.array(trk.last), status
    out = np.array(trk.last)
    if mode == MOTION_MODEL:
        Tlr = mat44(trk.trajectory[-1]["pose"])                      # mlTrajectory.back().mRelativeFramePose (:796)
        T = mul44(Tlr, mat44(kf_pose[trk.last_ref]["Tcw"]), rules, literal)   # Tlr*pRef->GetPose() (:798)
        trk.last["Tcw"] = T[:3].reshape(12)
        trk.last["Ow"] = set_pose_ow(trk.last["Tcw"], rules, literal)
        T = mul44(mat44(trk.velocity), mat44(trk.last["Tcw"]), rules, literal)   # mVelocity*mLastFrame.mTcw (:866)
        out = np.array(trk.last)
        out["Tcw"] = T[:3].reshape(12)
        out["Ow"] = set_pose_ow(out["Tcw"], rules, literal)
    return out, 0


def commit(trk, pose, ok, ref_kf, frame_time, frame_id, kf_pose, cap, rules=REFERENCE, literal=False):
    """the end of Track(); returns the status (FULL | BAD_INDEX: nothing changed)"""
    status = (FULL if len(trk.trajectory) >= cap else 0) | (0 if 0 <= ref_kf < len(kf_pose) else BAD_INDEX)
    if status:
        return status
    pose = np.array(pose, KF_POSE_DTYPE).reshape(())
    Tcw = mat44(pose["Tcw"])
    if ok:                                                          # :429
        if trk.has_last:                                            # !mLastFrame.mTcw.empty() (:432)
            LastTwc = pose_inverse(trk.last["Tcw"], trk.last["Ow"])  # :434-436
            trk.velocity = mul44(Tcw, LastTwc, rules, literal)[:3].reshape(12)   # :437
            trk.has_velocity = True
        else:
            trk.velocity, trk.has_velocity = np.zeros(12, f32), False   # mVelocity = cv::Mat() (:440)
    elif rules.lost_velocity == "clear":
        trk.velocity, trk.has_velocity = np.zeros(12, f32), False
    trk.last, trk.has_last, trk.last_ref = pose, True, int(ref_kf)  # mLastFrame = Frame(mCurrentFrame) (:493)
    r = np.zeros((), TRAJECTORY_RECORD_DTYPE)                       # :497-506
    r["ref_kf"], r["frame_time"], r["frame_id"], r["lost"], r["has_pose"] = ref_kf, frame_time, frame_id, not ok, 1
    r["pose"] = mul44(Tcw, pose_inverse(kf_pose[ref_kf]["Tcw"], kf_pose[ref_kf]["Ow"]), rules, literal)[:3].reshape(12)
    trk.trajectory.append(r)
    return 0


# ---------------------------------------------------------------- mTcp
def keyframe_tcp(pose, parent, record, nlist, tcp, rules=REFERENCE, literal=False, limit=False):
    """mTcp of the culled members of a KeyFrameCulling list: (tcp afterwards, info)"""
    out, info = np.array(tcp, f32).reshape(-1, 12), np.zeros(TCP_INFO, np.int32)
    nkf = len(pose)
    if limit:
        return out, info
    for g in range(max(0, min(int(nlist), len(record)))):
        a, action = int(record[g][0]), int(record[g][3])
        if action != CULLED:
            continue
        p = int(parent[a]) if 0 <= a < nkf else -1
        if not 0 <= p < nkf:
            info[2] += 1
            continue
        out[a] = mul44(mat44(pose[a]["Tcw"]), pose_inverse(pose[p]["Tcw"], pose[p]["Ow"]), rules, literal)[:3].reshape(12)
        info[1] += 1
    return out, info


# ---------------------------------------------------------------- GetTrajectory
def origin_of(kf_bad, kf_id, rules=REFERENCE):
    """vpKFs[0] of GetAllKeyFrames() sorted by lId: erased key frames are not in the map; -1 = the map is empty"""
    if rules.origin == "index0":
        return 0 if len(kf_bad) else -1
    live = [(int(kf_id[k]), k) for k in range(len(kf_bad)) if not kf_bad[k]]
    return min(live)[1] if live else -1


def chain_depth(c, i):
    """the number of culled key frames record i walks over, or -1 when the walk breaks"""
    k, d, nkf = int(c["traj"][i]["ref_kf"]), 0, len(c["pose"])
    while True:
        if not 0 <= k < nkf or d >= nkf:
            return -1
        if not c["kf_bad"][k]:
            return d
        k, d = int(c["parent"][k]), d + 1


def _bmat(rows):
    T = np.zeros((len(rows), 4, 4), f32)
    T[:, :3, :] = np.asarray(rows, f32).reshape(-1, 3, 4)
    T[:, 3, 3] = 1
    return T


def _bmul(A, B):
    """mul44 over a batch [m][4][4]: the same four float32 operations per element, in the same order"""
    s = A[:, :, 0:1] * B[:, 0:1, :]
    s = s + A[:, :, 1:2] * B[:, 1:2, :]
    s = s + A[:, :, 2:3] * B[:, 2:3, :]
    return s + A[:, :, 3:4] * B[:, 3:4, :]


def get_trajectory_batched(c, n=None):
    """get_trajectory under REFERENCE with the records side by side (for the large case): the walk advances every record still on a
    culled key frame by one product per round; np.sqrt of a float64 is correctly rounded like math.sqrt"""
    pose, bad, parent, tcp, traj = c["pose"], np.asarray(c["kf_bad"]), np.asarray(c["parent"], np.int64), np.asarray(c["tcp"], f32), c["traj"]
    nkf = len(pose)
    n = len(traj) if n is None else min(n, len(traj))
    traj = traj[:n]
    info = np.zeros(TRAJ_INFO, np.int32)
    o = origin_of(bad, c["kf_id"])
    info[1], info[3] = o, n
    if o < 0:
        info[0] = NO_ORIGIN
        return dict(info=info)
    with np.errstate(all="ignore"):
        us = traj["frame_time"].astype(f64) * f64(1e6)
        good = np.isfinite(us) & (us >= -2.0 ** 63) & (us < 2.0 ** 63)
        tu = np.where(good, np.trunc(np.where(good, us, 0.0)), 0.0).astype(np.int64)
        tu[~good] = INT64_MIN
        status = np.where(good, 0, BAD_TIME).astype(np.int32)
        lost = traj["lost"] != 0
        okay = ~lost & (traj["has_pose"] != 0)
        active = okay.copy()
        k = traj["ref_kf"].astype(np.int64)
        T = np.tile(eye44(), (n, 1, 1))
        for step in range(nkf + 1):
            brk = active & ((k < 0) | (k >= nkf) | (step >= nkf))
            okay &= ~brk
            active &= ~brk
            idx = np.nonzero(active)[0]
            idx = idx[bad[k[idx]] != 0]
            active[:] = False
            active[idx] = True
            if not len(idx):
                break
            T[idx] = _bmul(T[idx], _bmat(tcp[k[idx]]))
            k[idx] = parent[k[idx]]
        g = np.nonzero(okay)[0]
        Two = pose_inverse(pose[o]["Tcw"], pose[o]["Ow"])[None]
        Tc = _bmul(_bmat(traj["pose"][g]), _bmul(_bmul(T[g], _bmat(pose["Tcw"][k[g]])), Two))
        m = np.transpose(Tc[:, :3, :3], (0, 2, 1)).astype(f64)
        q = np.zeros((len(g), 4), f64)
        tr = (m[:, 0, 0] + m[:, 1, 1]) + m[:, 2, 2]
        i = np.where(m[:, 1, 1] > m[:, 0, 0], 1, 0)
        i = np.where(m[:, 2, 2] > np.where(i == 1, m[:, 1, 1], m[:, 0, 0]), 2, i)
        sel = tr > 0
        t = np.sqrt(tr + 1.0)
        q[sel, 0] = (0.5 * t)[sel]
        t = 0.5 / t
        for a, (r1, c1, r2, c2) in enumerate(((2, 1, 1, 2), (0, 2, 2, 0), (1, 0, 0, 1))):
            q[sel, 1 + a] = ((m[:, r1, c1] - m[:, r2, c2]) * t)[sel]
        for b in range(3):
            j, kk = (b + 1) % 3, (b + 2) % 3
            sel = ~(tr > 0) & (i == b)
            t = np.sqrt(((m[:, b, b] - m[:, j, j]) - m[:, kk, kk]) + 1.0)
            q[sel, 1 + b] = (0.5 * t)[sel]
            t = 0.5 / t
            q[sel, 0] = ((m[:, kk, j] - m[:, j, kk]) * t)[sel]
            q[sel, 1 + j] = ((m[:, j, b] + m[:, b, j]) * t)[sel]
            q[sel, 1 + kk] = ((m[:, kk, b] + m[:, b, kk]) * t)[sel]
        s = (Tc[:, 0, :3] * Tc[:, 0, 3:4] + Tc[:, 1, :3] * Tc[:, 1, 3:4]) + Tc[:, 2, :3] * Tc[:, 2, 3:4]
        tt = (s.astype(f64) * f64(-1.0)).astype(f32).astype(f64)
    out = dict(quat_wxyz=np.zeros((n, 4), f64), translation=np.zeros((n, 3), f64), time_usec=tu, frame_id=traj["frame_id"].astype(np.int64),
               is_lost=lost.astype(np.uint8), status=status, info=info)
    out["quat_wxyz"][g], out["translation"][g] = q, tt
    broken = ~lost & ~okay
    out["status"][broken] |= BROKEN
    info[2] = int(broken.sum())
    return out


def get_trajectory(c, rules=REFERENCE, literal=False, hits=None, n=None):
    """System::GetTrajectory over the first n records of case c (a dict: pose, kf_bad, parent, kf_id, tcp, traj).  Returns a dict:
    quat_wxyz, translation, time_usec, frame_id, is_lost, status, info; with no live key frame only info."""
    pose, bad, parent, tcp, traj = c["pose"], c["kf_bad"], c["parent"], c["tcp"], c["traj"]
    nkf = len(pose)
    n = len(traj) if n is None else min(n, len(traj))
    info = np.zeros(TRAJ_INFO, np.int32)
    o = origin_of(bad, c["kf_id"], rules)
    info[1], info[3] = o, n
    if o < 0:
        info[0] = NO_ORIGIN
        return dict(info=info)
    Two = pose_inverse(pose[o]["Tcw"], pose[o]["Ow"])               # :379
    out = dict(quat_wxyz=np.zeros((n, 4), f64), translation=np.zeros((n, 3), f64), time_usec=np.zeros(n, np.int64), frame_id=np.zeros(n, np.int64),
               is_lost=np.zeros(n, np.uint8), status=np.zeros(n, np.int32), info=info)
    for i in range(n):
        r = traj[i]
        out["time_usec"][i], good = time_usec(r["frame_time"], rules)
        if not good:
            out["status"][i] |= BAD_TIME
        out["frame_id"][i], out["is_lost"][i] = r["frame_id"], 1 if r["lost"] else 0
        if r["lost"]:                                               # :388-390: Pose() is value-initialised
            _hit(hits, "lost")
            continue
        okay, k, steps = bool(r["has_pose"]), int(r["ref_kf"]), 0
        Trw = eye44()                                               # :394
        first = True
        while okay:                                                 # :397-400
            if not 0 <= k < nkf or steps >= nkf:
                okay = False
                break
            if not bad[k]:
                break
            if first and not rules.identity_product:
                Trw = mat44(tcp[k])
            else:
                Trw = mul44(Trw, mat44(tcp[k]), rules, literal)
            first = False
            k, steps = int(parent[k]), steps + 1
        if not okay:
            out["status"][i] |= BROKEN
            info[2] += 1
            continue
        _hit(hits, "depth_%d" % min(steps, 3))
        rel, Tk = mat44(r["pose"]), mat44(pose[k]["Tcw"])
        if rules.grouping == "left":
            Trw = mul44(mul44(Trw, Tk, rules, literal), Two, rules, literal)   # Trw*pKF->GetPose()*Two (:402)
            Tcw = mul44(rel, Trw, rules, literal)                   # :404
        else:
            Tcw = mul44(rel, mul44(Trw, mul44(Tk, Two, rules, literal), rules, literal), rules, literal)
        R = Tcw[:3, :3] if rules.quat_of == "block" else Tcw[:3, :3].T   # :405
        _hit(hits, "quat_" + quat_branch(R.astype(f64)))
        out["quat_wxyz"][i] = quat_wxyz(R.astype(f64))               # :406
        out["translation"][i] = set_pose_ow(Tcw[:3].reshape(12), rules, literal).astype(f64)   # :407-409
    return out
