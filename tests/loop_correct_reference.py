"""A literal object-level restatement of the two map rewrites of loop closing (thirdparty/orb-slam2/src/LoopClosing.cc):

  correct_loop        CorrectLoop's propagation, :438-516 (without the UpdateConnections of :515): a dict keyed by ADDRESS for
                      CorrectedSim3 / NonCorrectedSim3, sequential loops, one mnCorrectedByKF per point, SetPose after each key
                      frame's point loop, UpdateNormalAndDepth on the objects as they stand at that moment
  update_map          the map update of RunGlobalBundleAdjustment, :679-742: a deque for lpKFtoCheck, children sets, mTcwGBA /
                      mTcwBefGBA per key frame, then the point loop
  correct_loop_claims, update_map_chains   the restatements the kernels use (a first claim by address rank; a chain walked up and
                      multiplied down per key frame), for tests/test_loop_correction.py to compare with the literal sequences

numpy float32 / float64 in the sources' operation order.  The Sim3 and quaternion arithmetic is tests/optsim3_reference.py's and
tests/pose_reference.py's, UpdateNormalAndDepth tests/map_point_reference.py's, [R | t/s] with SetPose's Ow tests/eg_reference.py's.
`rules` (a Rules) switches one reading or rule at a time; `hits` (a dict) counts the branches taken, as in tests/eg_reference.py.
The cases are the dicts tests/loop_correct_cases.py builds."""
import os
import sys
from collections import deque
from dataclasses import dataclass, replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eg_reference as EG  # noqa: E402
import map_point_reference as MPR  # noqa: E402
from optsim3_reference import Sim3, sim3_inverse, sim3_mul  # noqa: E402
from matcher_cases import SF  # noqa: E402
from pose_reference import quat_from_matrix  # noqa: E402
from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE, SIM3D_DTYPE  # noqa: E402

f32, f64 = np.float32, np.float64
OVER_OBS, BAD_INDEX, LC_INFO, MU_INFO = 1, 2, 4, 4                 # PGORB_LC_*, PGORB_MU_INFO (include/pgorb.h)
MAX_OBS = MPR.MAX_OBS


@dataclass(frozen=True)
class Rules:
    claim_order: str = "address"        # the point loop runs over a std::map<KeyFrame*, ..> (:472) | "index"
    once: bool = True                   # mnCorrectedByKF == mpCurrentKF->mnId skips a point (:488) | False: corrected by every holder
    divide_t_by_s: bool = True          # eigt *= (1./s) (:508)
    cur_is_scw: bool = True             # CorrectedSim3[mpCurrentKF] = mg2oScw (:439) | False: composed like the others
    centres: str = "as_they_stand"      # UpdateNormalAndDepth reads the key frames as they are at :500 | "all_corrected" |
                                        # "own_corrected": the corrector's own SetPose before its point loop | "as_passed": no
                                        # SetPose before the last point loop has ended
    done_child: str = "keep"            # a child with mnBAGlobalForKF == nLoopKF keeps its mTcwGBA (:690) | "recompute"
    grouping: str = "left"              # (Tchild*Twc)*TcwGBA (:692-693) | "right": Tchild*(Twc*TcwGBA)
    parent_pose: str = "before"         # Twc = pKF->GetPoseInverse() before pKF's SetPose (:686, :701) | "after"
    ref_visited: bool = True            # pRefKF->mnBAGlobalForKF != nLoopKF -> continue (:725) | False: moved by the adjusted flag alone
    done_point: str = "copy"            # SetWorldPos(mPosGBA) (:718) | "transform": moved through the reference key frame too


REFERENCE = Rules()
MUTANTS = {
    "claim_index_order": replace(REFERENCE, claim_order="index"),
    "corrected_twice": replace(REFERENCE, once=False),
    "t_not_divided_by_s": replace(REFERENCE, divide_t_by_s=False),
    "cur_composed": replace(REFERENCE, cur_is_scw=False),
    "all_centres_corrected": replace(REFERENCE, centres="all_corrected"),
    "own_centre_corrected": replace(REFERENCE, centres="own_corrected"),
    "all_centres_as_passed": replace(REFERENCE, centres="as_passed"),
    "done_child_recomputed": replace(REFERENCE, done_child="recompute"),
    "regrouped": replace(REFERENCE, grouping="right"),
    "parent_pose_after": replace(REFERENCE, parent_pose="after"),
    "ref_not_visited_moved": replace(REFERENCE, ref_visited=False),
    "done_point_transformed": replace(REFERENCE, done_point="transform"),
}


def _hit(hits, k):
    if hits is not None:
        hits[k] = hits.get(k, 0) + 1


# ---------------------------------------------------------------- cv::Mat and Converter
def mat44(Tcw):
    """the 4 x 4 CV_32F matrix of pose rows [12]"""
    T = np.zeros((4, 4), f32)
    T[:3, :] = np.asarray(Tcw, f32).reshape(3, 4)
    T[3, 3] = 1
    return T


def pose_inverse(Tcw, Ow):
    """KeyFrame::GetPoseInverse(): Twc = [Rcw' | Ow] with Ow as stored"""
    T = mat44(Tcw)
    W = np.zeros((4, 4), f32)
    W[:3, :3] = T[:3, :3].T
    W[:3, 3] = np.asarray(Ow, f32)
    W[3, 3] = 1
    return W


def mul44(A, B):
    """cv::Mat A*B, 4 x 4 CV_32F: gemm's small-matrix path (len 4), the four terms in index order in float, every term formed"""
    Cm = np.zeros((4, 4), f32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                s = f32(f32(A[r, 0] * B[0, c]) + f32(A[r, 1] * B[1, c]))
                s = f32(s + f32(A[r, 2] * B[2, c]))
                Cm[r, c] = f32(s + f32(A[r, 3] * B[3, c]))
    return Cm


def quat_branch(R):
    """the branch Eigen's Quaterniond(Matrix3d) takes: 'trace', 'x', 'y' or 'z'"""
    if (R[0, 0] + R[1, 1]) + R[2, 2] > 0:
        return "trace"
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return "xyz"[i]


def sim3_of(T, hits=None):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of the 4 x 4 float matrix T"""
    R = np.asarray(T, f32)[:3, :3].astype(f64)
    _hit(hits, "quat_" + quat_branch(R))
    return Sim3(quat_from_matrix(R), np.asarray(T, f32)[:3, 3].astype(f64), 1.0)


def to_pose(S, rules=REFERENCE):
    """[R | t/s] (:504-510) through Converter::toCvSE3 to float, then SetPose's Ow: (Tcw [12], Ow [3])"""
    return EG.to_pose(S, replace(EG.REFERENCE, divide_t_by_s=rules.divide_t_by_s))


def set_pose_ow(Tcw):
    """KeyFrame::SetPose's Ow = -Rcw.t()*tcw: gemm's small-matrix path times alpha = -1 in double"""
    T = np.asarray(Tcw, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.array([f32(f64(f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3]))) * f64(-1.0)) for i in range(3)], f32)


def rt_row(r, t, p):
    """one row of R*p + t: float sums, then (float)(sum + t) in double (t folded into gemm's C)"""
    with np.errstate(all="ignore"):
        return f32(f64(f32(f32(f32(r[0] * p[0]) + f32(r[1] * p[1])) + f32(r[2] * p[2]))) + f64(t))


# ---------------------------------------------------------------- the objects
class KeyFrame(MPR.KeyFrame):
    def __init__(self, idx, addr, pose, octaves):
        keys = np.zeros(len(octaves), [("octave", "<i4")])
        keys["octave"] = octaves
        super().__init__(keys, np.zeros((max(len(octaves), 1), 32), np.uint8), pose["Ow"])
        self.idx, self.addr = idx, addr
        self.Tcw = np.array(pose["Tcw"], f32)
        self.slots = []                                             # GetMapPointMatches(): MapPoint or None


class MapPoint(MPR.MapPoint):
    def __init__(self, idx, rec, bad):
        super().__init__(rec["pos"], np.zeros(32, np.uint8), rec["normal"], rec["min_distance"], rec["max_distance"], bad)
        self.idx = idx
        self.corrected_by_kf, self.corrected_reference = -1, -1     # mnCorrectedByKF (-1: no loop yet), mnCorrectedReference


def rank_of(case, f):
    return int(case["kf_order"][f]) if case["kf_order"] is not None else f


def members_of(case):
    """mvpCurrentConnectedKFs as the library reads the list: entries that are negative, out of range or cur_kf are skipped, one
    named twice counts once, cur_kf is pushed at the back (:435-436)"""
    nkf, cur, out = case["nkf"], case["cur_kf"], []
    for f in case["list"]:
        f = int(f)
        if 0 <= f < nkf and f != cur and f not in out:
            out.append(f)
    return out + [cur]


def build(case):
    kfs = [KeyFrame(f, rank_of(case, f), case["pose"][f], case["octaves"][f]) for f in range(case["nkf"])]
    pb = case["point_bad"]
    mps = [MapPoint(p, case["points"][p], bool(pb[p]) if pb is not None else False) for p in range(case["npoints"])]
    for f, kf in enumerate(kfs):
        kf.slots = [mps[p] if p >= 0 else None for p in case["kf_point"][f]]
    st = case["obs_start"]
    for p, mp in enumerate(mps):
        mp.obs = [(kfs[case["obs_frame"][k]], int(case["obs_idx"][k])) for k in range(st[p], st[p + 1])]
        mp.ref = mp.obs[case["ref_obs"][p]][0] if mp.obs and 0 <= case["ref_obs"][p] < len(mp.obs) else None
    return kfs, mps


def _export_loop(case, kfs, mps, corrected, non_corrected, over):
    nkf, n = case["nkf"], case["npoints"]
    out = dict(has_corrected=np.zeros(nkf, np.uint8), corrected=np.zeros(nkf, SIM3D_DTYPE), has_non_corrected=np.zeros(nkf, np.uint8),
               non_corrected=np.zeros(nkf, SIM3D_DTYPE), pose_out=np.array(case["pose"], KF_POSE_DTYPE), points=np.zeros(n, MAP_POINT_DTYPE),
               corrected_by=np.full(n, -1, np.int32), point_ref_kf=np.array(case["ref_kf"], np.int32).copy())
    for name, table in (("corrected", corrected), ("non_corrected", non_corrected)):
        for kf in kfs:
            if kf.addr in table:
                S = table[kf.addr]
                out["has_" + name][kf.idx] = 1
                out[name][kf.idx]["r"], out[name][kf.idx]["t"], out[name][kf.idx]["s"] = S.q, S.t, S.s
    for kf in kfs:
        out["pose_out"][kf.idx]["Tcw"], out["pose_out"][kf.idx]["Ow"] = kf.Tcw, kf.Ow
    ncor = 0
    for mp in mps:
        r = out["points"][mp.idx]
        r["pos"], r["normal"], r["min_distance"], r["max_distance"] = mp.pos, mp.normal, mp.min_d, mp.max_d
        if mp.corrected_reference >= 0:
            out["corrected_by"][mp.idx] = out["point_ref_kf"][mp.idx] = mp.corrected_reference
            ncor += 1
    out["info"] = np.array([OVER_OBS if over else 0, len(corrected), ncor, over], np.int32)
    return out


# ---------------------------------------------------------------- LoopClosing.cc:438-516
def correct_loop(case, rules=REFERENCE, hits=None, sf=None, nlevels=8):
    """The literal sequence.  Returns the dict of outputs include/pgorb.h names."""
    sf = SF if sf is None else sf
    kfs, mps = build(case)
    cur = kfs[case["cur_kf"]]
    loop_id = 1                                                     # mpCurrentKF->mnId: any value no point carries yet
    scw = EG.sim3_from_record(case["scw"])
    connected = [kfs[f] for f in members_of(case)]                  # :435-436
    by_addr = {kf.addr: kf for kf in kfs}
    corrected, non_corrected = {}, {}                               # KeyFrameAndPose: std::map<KeyFrame*, g2o::Sim3>
    corrected[cur.addr] = scw                                       # :439
    Twc = pose_inverse(cur.Tcw, cur.Ow)                             # :440
    for kfi in connected:                                           # :447-469
        Tiw = mat44(kfi.Tcw)
        if kfi is not cur or not rules.cur_is_scw:
            Tic = mul44(Tiw, Twc)                                   # :455
            corrected[kfi.addr] = sim3_mul(sim3_of(Tic, hits), scw)  # :458-461
        non_corrected[kfi.addr] = sim3_of(Tiw, hits)                # :464-468
    new_pose = {a: to_pose(S, rules) for a, S in corrected.items()}
    if rules.centres == "all_corrected":
        for a, (T, Ow) in new_pose.items():
            by_addr[a].Ow = Ow
    over = 0
    keys = sorted(corrected) if rules.claim_order == "address" else [kf.addr for kf in sorted((by_addr[a] for a in corrected), key=lambda k: k.idx)]
    for a in keys:                                                  # :472-516, a std::map: address order
        kfi, Siw_c = by_addr[a], corrected[a]
        Swi_c = sim3_inverse(Siw_c)                                 # :476
        Siw = non_corrected[a]                                      # :478
        if rules.centres == "own_corrected":
            kfi.Ow = new_pose[a][1]
        for mp in kfi.slots:                                        # :481-501
            if mp is None or mp.bad:
                continue
            if rules.once and mp.corrected_by_kf == loop_id:        # :488
                _hit(hits, "already_corrected")
                continue
            P = EG.sim3_map(Swi_c, EG.sim3_map(Siw, mp.pos.astype(f64)))         # :492-494
            mp.pos = P.astype(f32)                                  # :496-497
            mp.corrected_by_kf, mp.corrected_reference = loop_id, kfi.idx       # :498-499
            if len(mp.obs) > MAX_OBS:                               # the library's limit; the reference has none
                over += 1
            else:
                MPR.update_normal_and_depth(mp, sf, nlevels)        # :500
        kfi.Tcw = new_pose[a][0]                                    # :504-512
        if rules.centres != "as_passed":
            kfi.Ow = new_pose[a][1]
    for a in keys:
        by_addr[a].Ow = new_pose[a][1]
    return _export_loop(case, kfs, mps, corrected, non_corrected, over)


def correct_loop_claims(case, sf=None, nlevels=8):
    """What the kernels do: the Sim3s and poses per member; per point the smallest address rank among the members that hold it in a
    slot; per claimed point the map and UpdateNormalAndDepth with the centre rule (a member of a strictly smaller rank than the
    corrector contributes its corrected centre)."""
    sf = SF if sf is None else sf
    kfs, mps = build(case)
    cur = kfs[case["cur_kf"]]
    scw = EG.sim3_from_record(case["scw"])
    Twc = pose_inverse(cur.Tcw, cur.Ow)
    corrected, non_corrected, new_pose = {}, {}, {}
    for f in members_of(case):
        kf = kfs[f]
        corrected[kf.addr] = scw if kf is cur else sim3_mul(sim3_of(mul44(mat44(kf.Tcw), Twc)), scw)
        non_corrected[kf.addr] = sim3_of(mat44(kf.Tcw))
        new_pose[kf.addr] = to_pose(corrected[kf.addr])
    by_addr = {kf.addr: kf for kf in kfs}
    claim = {}
    for a in corrected:
        for mp in by_addr[a].slots:
            if mp is not None and not mp.bad:
                claim[mp.idx] = min(claim.get(mp.idx, a), a)
    old_ow = {kf.addr: kf.Ow.copy() for kf in kfs}
    over = 0
    for p, a in claim.items():
        mp = mps[p]
        mp.pos = EG.sim3_map(sim3_inverse(corrected[a]), EG.sim3_map(non_corrected[a], mp.pos.astype(f64))).astype(f32)
        mp.corrected_reference = by_addr[a].idx
        if len(mp.obs) > MAX_OBS:
            over += 1
            continue
        for kf, _ in mp.obs:
            kf.Ow = new_pose[kf.addr][1] if kf.addr in corrected and kf.addr < a else old_ow[kf.addr]
        MPR.update_normal_and_depth(mp, sf, nlevels)
    for a, (T, Ow) in new_pose.items():
        by_addr[a].Tcw, by_addr[a].Ow = T, Ow
    for kf in kfs:
        if kf.addr not in corrected:
            kf.Ow = old_ow[kf.addr]
    return _export_loop(case, kfs, mps, corrected, non_corrected, over)


# ---------------------------------------------------------------- LoopClosing.cc:679-742
class GbaKeyFrame:
    def __init__(self, idx, pose, gba, done, bad):
        self.idx, self.bad = idx, bool(bad)
        self.Tcw, self.Ow = np.array(pose["Tcw"], f32), np.array(pose["Ow"], f32)
        self.done = bool(done)                                      # mnBAGlobalForKF == nLoopKF
        self.has_gba = self.done                                    # mTcwGBA holds a value of THIS adjustment (the library's departure)
        self.TcwGBA = np.array(gba["Tcw"], f32) if done else None
        self.gba_record = gba
        self.TcwBefGBA, self.OwBefGBA = None, None
        self.childs, self.updated, self.recomputed = [], False, False


def _children(case, kfs):
    """GetChilds(): a bad key frame is nobody's child and has none (SetBadFlag re-parents them); an origin has no parent"""
    for k in kfs:
        p = int(case["parent"][k.idx])
        if 0 <= p < len(kfs) and p != k.idx and not k.bad and not kfs[p].bad and not case["kf_origin"][k.idx]:
            kfs[p].childs.append(k)                                 # a std::set<KeyFrame*>: the order decides nothing here


def _export_map(case, kfs, pos, pupd):
    out = dict(pose_out=np.array(case["pose"], KF_POSE_DTYPE), kf_updated=np.zeros(case["nkf"], np.uint8),
               points=np.array(case["points"], MAP_POINT_DTYPE), point_updated=np.array(pupd, np.uint8))
    for k in kfs:
        if k.updated:
            out["kf_updated"][k.idx] = 1
            if k.recomputed:
                out["pose_out"][k.idx]["Tcw"], out["pose_out"][k.idx]["Ow"] = k.Tcw, k.Ow
            else:
                out["pose_out"][k.idx] = k.gba_record
    out["points"]["pos"] = pos
    out["info"] = np.array([0, int(out["kf_updated"].sum()), sum(k.updated and k.recomputed for k in kfs), int(out["point_updated"].sum())], np.int32)
    return out


def _move_points(case, kfs, rules):
    n = case["npoints"]
    pos, upd = np.array(case["points"]["pos"], f32).reshape(n, 3).copy(), np.zeros(n, np.uint8)
    pb = case["point_bad"]
    for p in range(n):                                              # :706-742
        if pb is not None and pb[p]:
            continue
        if case["point_done"][p] and rules.done_point == "copy":    # :715-719
            pos[p] = case["pos_gba"][p]
            upd[p] = 1
            continue
        r = int(case["ref_kf"][p])
        if not 0 <= r < len(kfs):
            continue                                                # no reference key frame: kept (the reference would dereference it)
        ref = kfs[r]
        if not (ref.updated or (not rules.ref_visited and ref.done and not ref.bad)):       # :725
            continue
        if ref.updated:
            Tb, Tn, On = ref.TcwBefGBA.reshape(3, 4), ref.Tcw.reshape(3, 4), ref.Ow
        else:                                                       # (mutant only) never visited: both poses are the one passed in
            Tb = Tn = ref.Tcw.reshape(3, 4)
            On = ref.Ow
        Xc = [rt_row(Tb[k, :3], Tb[k, 3], pos[p]) for k in range(3)]             # :729-731
        pos[p] = [rt_row(Tn[:3, k], On[k], Xc) for k in range(3)]                # :734-738: Rwc = Rcw', twc = Ow
        upd[p] = 1
    return pos, upd


def update_map(case, rules=REFERENCE, hits=None):
    """The literal sequence, with the library's one departure: a key frame whose mTcwGBA holds no value of this adjustment is not
    updated (the reference would read a stale matrix)."""
    kfs = [GbaKeyFrame(k, case["pose"][k], case["pose_gba"][k], case["kf_done"][k], case["kf_bad"][k] if case["kf_bad"] is not None else 0)
           for k in range(case["nkf"])]
    _children(case, kfs)
    to_check = deque(k for k in kfs if case["kf_origin"][k.idx] and not k.bad)   # :680
    while to_check:                                                 # :682-703
        kf = to_check[0]
        Twc = pose_inverse(kf.Tcw, kf.Ow)                           # :686
        for ch in kf.childs:
            if not ch.done or rules.done_child == "recompute":      # :690
                if kf.has_gba:
                    Tp = mat44(kf.TcwGBA)
                    if rules.parent_pose == "after":
                        Twc = pose_inverse(kf.TcwGBA, kf.gba_record["Ow"] if not kf.recomputed else set_pose_ow(kf.TcwGBA))
                    if rules.grouping == "left":
                        T = mul44(mul44(mat44(ch.Tcw), Twc), Tp)    # :692-693
                    else:
                        T = mul44(mat44(ch.Tcw), mul44(Twc, Tp))
                    ch.TcwGBA, ch.has_gba, ch.recomputed = T[:3, :].reshape(12).copy(), True, True
                    _hit(hits, "recomputed")
                else:
                    _hit(hits, "stale_parent")
            to_check.append(ch)                                     # :697
        if kf.has_gba:
            kf.TcwBefGBA, kf.OwBefGBA = kf.Tcw, kf.Ow               # :700
            kf.Tcw = kf.TcwGBA                                      # :701 SetPose(mTcwGBA)
            kf.Ow = set_pose_ow(kf.Tcw) if kf.recomputed else np.array(kf.gba_record["Ow"], f32)
            kf.updated = True
        to_check.popleft()
    pos, upd = _move_points(case, kfs, rules)
    return _export_map(case, kfs, pos, upd)


def update_map_chains(case):
    """What the kernels do: per key frame walk up to the first origin (a bad key frame or more than nkf steps end the walk), take the
    nearest adjusted key frame of the chain, and multiply down the chain from it in order."""
    nkf = case["nkf"]
    bad = lambda k: case["kf_bad"] is not None and bool(case["kf_bad"][k])
    kfs = [GbaKeyFrame(k, case["pose"][k], case["pose_gba"][k], case["kf_done"][k], bad(k)) for k in range(nkf)]
    for k in range(nkf):
        if bad(k):
            continue
        chain, cur, reached, done_at = [k], k, False, -1
        while True:
            if done_at < 0 and case["kf_done"][cur]:
                done_at = len(chain) - 1
            if case["kf_origin"][cur]:
                reached = True
                break
            p = int(case["parent"][cur])
            if p < 0 or p >= nkf or bad(p) or len(chain) >= nkf:
                break
            chain.append(p)
            cur = p
        if not (reached and done_at >= 0):
            continue
        kf = kfs[k]
        kf.updated = True
        if done_at == 0:
            continue
        T = mat44(case["pose_gba"][chain[done_at]]["Tcw"])
        for lvl in range(done_at - 1, -1, -1):
            c, par = chain[lvl], chain[lvl + 1]
            T = mul44(mul44(mat44(case["pose"][c]["Tcw"]), pose_inverse(case["pose"][par]["Tcw"], case["pose"][par]["Ow"])), T)
        kf.recomputed, kf.TcwGBA = True, T[:3, :].reshape(12).copy()
    for kf in kfs:
        if kf.updated:
            kf.TcwBefGBA, kf.OwBefGBA = kf.Tcw, kf.Ow
            if kf.recomputed:
                kf.Tcw, kf.Ow = kf.TcwGBA, set_pose_ow(kf.TcwGBA)
            else:
                kf.Tcw, kf.Ow = np.array(kf.gba_record["Tcw"], f32), np.array(kf.gba_record["Ow"], f32)
    pos, upd = _move_points(case, kfs, REFERENCE)
    return _export_map(case, kfs, pos, upd)
