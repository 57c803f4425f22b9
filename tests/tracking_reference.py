"""A plain, sequential restatement of the tracking thread's three projection searches, front part included (thirdparty/orb-slam2):
  Tracking::SearchLocalPoints (src/Tracking.cc:1134-1184) with Frame::isInFrustum (src/Frame.cc:273-329) and
      ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:46-131);
  ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) (src/ORBmatcher.cc:1326-1474);
  ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1476-1603).
It is written from that upstream text and the float readings of DESIGN.md section 4 (numpy float32 / float64 scalars, one rounding
per step; the cv::Mat helpers of tests/mapping_reference.py, the grid, PredictScale and histogram helpers of
tests/matcher_reference.py); it does not use oracle/ and was not derived from the HIP kernels (pilotguru_amd/csrc/track.hip).

Objects are real: a MapPoint carries its pose fields, descriptor, bad flag, Observations() > 0 and the mutable tracking fields
(mnLastFrameSeen, mbTrackInView, mTrackProjX, ...); a Frame carries keypoints, descriptors, the grid, pose and slots.  `rules` (a
Rules) switches one reading or rule at a time; `hits` (a collections.Counter or None) counts the edges reached.  Where the
reference would convert a NaN projection to int inside GetFeaturesInArea (undefined), the point is skipped, as include/pgorb.h
states."""
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_reference as MR  # noqa: E402
import matcher_reference as R  # noqa: E402
from matcher_reference import HISTO_LENGTH, TH_HIGH, Grid, _dist, _hit, predict_scale  # noqa: E402

f32, f64 = np.float32, np.float64


@dataclass(frozen=True)
class Rules:
    gemm: str = "float"                  # mRcw*P + mtcw on gemm's small-matrix path (float sums) | "double"
    norm: str = "double"                 # cv::norm(PO): double sum, double sqrt | "float"
    dot: str = "double"                  # PO.dot(Pn): double sum | "float"
    viewcos_div: str = "double"          # PO.dot(Pn)/dist divided in double, rounded once | "float": both rounded first
    frame_bounds: str = "inclusive"      # u < mnMinX || u > mnMaxX rejects | "strict": the bounds themselves reject too
    reloc_depth_sign: str = "off"        # the key-frame form has no depth-sign test | "on": invzc < 0 skips
    last_frame_bad_skip: str = "off"     # the last-frame form has no isBad() test | "on": a bad point is skipped
    bad_slot: str = "cleared"            # SearchLocalPoints clears a slot holding a bad point | "keeps_keypoint"
    seen: str = "skipped"                # a query with mnLastFrameSeen == this frame is skipped | "ignored"


REFERENCE = Rules()
MUTANTS = {
    "gemm=double": Rules(gemm="double"),
    "norm=float": Rules(norm="float"),
    "dot=float": Rules(dot="float"),
    "viewcos_div=float": Rules(viewcos_div="float"),
    "frame_bounds=strict": Rules(frame_bounds="strict"),
    "reloc_depth_sign=on": Rules(reloc_depth_sign="on"),
    "last_frame_bad_skip=on": Rules(last_frame_bad_skip="on"),
    "bad_slot_keeps_keypoint": Rules(bad_slot="keeps_keypoint"),
    "seen_ignored": Rules(seen="ignored"),
}


class MapPoint:
    def __init__(self, pid, pos, normal, min_d, max_d, desc, bad=False, has_obs=True):
        self.id = pid
        self.pos = np.asarray(pos, np.float32).reshape(3)
        self.normal = np.asarray(normal, np.float32).reshape(3)
        self.min_d, self.max_d = f32(min_d), f32(max_d)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(32)
        self.dint = int.from_bytes(self.desc.tobytes(), "little")
        self.bad, self.has_obs = bool(bad), bool(has_obs)
        self.last_frame_seen = -1
        self.track_in_view = False
        self.proj_x = self.proj_y = self.view_cos = f32(0)
        self.level = 0


class Frame:
    """The slice of a Frame the three searches read: mnId, mvKeysUn, mDescriptors, the float bounds and grid, mTcw / mOw and the
    camera (a KF_POSE_DTYPE record), the scale tables, and mvpMapPoints."""

    def __init__(self, fid, keys, desc, bounds, pose, sf, log_sf, nlevels):
        self.id = fid
        self.keys = np.ascontiguousarray(keys)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.dint = R.descriptor_ints(self.desc)
        self.bounds = tuple(f32(b) for b in bounds)
        self.grid = Grid(self.keys, self.bounds)
        self.pose = pose
        self.sf, self.log_sf, self.nlevels = np.asarray(sf, np.float32), f32(log_sf), nlevels
        self.slots = [None] * len(self.keys)


_log_f = None


def _LOG_F():
    global _log_f
    if _log_f is None:
        _log_f = R.contract_log_f()
    return _log_f


def _edge(hits, name, val, bound):
    """Counts val exactly on `bound` and one ulp either side of it."""
    if hits is None or not np.isfinite(val):
        return
    val, bound = f32(val), f32(bound)
    if val == bound:
        _hit(hits, name + "_on")
    elif val == np.nextafter(bound, f32(-np.inf)):
        _hit(hits, name + "_ulp_below")
    elif val == np.nextafter(bound, f32(np.inf)):
        _hit(hits, name + "_ulp_above")


# ---------------------------------------------------------------- the front part
def to_camera(pose, pos, rules=REFERENCE):
    """Rcw*P + tcw: gemm's small-matrix path with tcw as gemm's C, folded in double and rounded once."""
    T = np.asarray(pose["Tcw"], np.float32).reshape(3, 4)
    p = np.asarray(pos, np.float32)
    if rules.gemm == "float":
        # d = (float)(s*alpha + c*beta): s the float sum of the three products, c = tcw; a -0.0 sum plus a -0.0 tcw stays -0.0
        # (MR.gemm3 is the form without C: its "+ 0.0" would turn it into +0.0)
        return [f32(f64(f32(f32(f32(T[r][0] * p[0]) + f32(T[r][1] * p[1])) + f32(T[r][2] * p[2]))) + f64(T[r][3])) for r in range(3)]
    return [f32(MR._sumprod(T[r][:3], p) + f64(T[r][3])) for r in range(3)]


def _z_hits(hits, z):
    if z == 0:
        _hit(hits, "z_neg_zero" if np.signbit(z) else "z_pos_zero")
    elif z < 0:
        _hit(hits, "z_negative")
    elif z < f32(1e-20):
        _hit(hits, "z_tiny")


def project(pose, pc, invz):
    """u = fx*xc*invz + cx, v = fy*yc*invz + cy: float, in the written order."""
    fx, fy, cx, cy = (f32(pose[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        u = f32(f32(f32(fx * pc[0]) * invz) + cx)
        v = f32(f32(f32(fy * pc[1]) * invz) + cy)
    return u, v


def in_bounds(frame, u, v, rules=REFERENCE, hits=None):
    """The Frame's bounds test (Frame.cc:295-298, ORBmatcher.cc:1377-1380, :1511-1514): inclusive on both sides.  A NaN
    projection is skipped (the reference's behaviour on it is undefined)."""
    mnx, mxx, mny, mxy = frame.bounds
    if np.isnan(u) or np.isnan(v):
        _hit(hits, "nan_projection")
        return False
    if np.isinf(u) or np.isinf(v):
        _hit(hits, "inf_projection")
    _edge(hits, "u_min", u, mnx); _edge(hits, "u_max", u, mxx); _edge(hits, "v_min", v, mny); _edge(hits, "v_max", v, mxy)
    if rules.frame_bounds == "strict":
        out = u <= mnx or u >= mxx or v <= mny or v >= mxy
    else:
        out = u < mnx or u > mxx or v < mny or v > mxy
    if out:
        _hit(hits, "outside_bounds")
    return not out


def dist_to_centre(pose, pos, rules=REFERENCE):
    """PO = P - Ow in float, cv::norm(PO) rounded once to float.  Returns (PO, dist)."""
    Ow = np.asarray(pose["Ow"], np.float32)
    p = np.asarray(pos, np.float32)
    PO = [f32(p[i] - Ow[i]) for i in range(3)]
    return PO, f32(MR.normd(PO, MR.Rules(norm=rules.norm)))


def _depth_ok(mp, dist, hits):
    """dist inside [GetMinDistanceInvariance(), GetMaxDistanceInvariance()] = [0.8f*mfMinDistance, 1.2f*mfMaxDistance]."""
    lo, hi = f32(f32(0.8) * mp.min_d), f32(f32(1.2) * mp.max_d)
    _edge(hits, "dist_min", dist, lo); _edge(hits, "dist_max", dist, hi)
    if dist < lo or dist > hi:
        _hit(hits, "depth_low" if dist < lo else "depth_high")
        return False
    return True


def _level(frame, mp, dist, hits):
    lvl = predict_scale(mp.max_d, dist, frame.log_sf, frame.nlevels, _LOG_F(), hits)
    with np.errstate(all="ignore"):
        if lvl == frame.nlevels - 1 and f32(mp.max_d / dist) > f32(frame.sf[frame.nlevels - 1] * frame.sf[1]):
            _hit(hits, "predict_scale_clamped_high")
    return lvl


def is_in_frustum(frame, mp, viewing_cos_limit, rules=REFERENCE, hits=None):
    """Frame::isInFrustum (Frame.cc:273-329)."""
    mp.track_in_view = False
    pc = to_camera(frame.pose, mp.pos, rules)
    _z_hits(hits, pc[2])
    if pc[2] < f32(0):
        return False
    with np.errstate(all="ignore"):
        invz = f32(f32(1) / pc[2])
    u, v = project(frame.pose, pc, invz)
    if not in_bounds(frame, u, v, rules, hits):
        return False
    PO, dist = dist_to_centre(frame.pose, mp.pos, rules)
    if not _depth_ok(mp, dist, hits):
        return False
    d = MR.dotd(PO, mp.normal, MR.Rules(norm=rules.dot))
    with np.errstate(all="ignore"):
        view_cos = f32(f32(d) / dist) if rules.viewcos_div == "float" else f32(f64(d) / f64(dist))
    lim = f32(viewing_cos_limit)
    _edge(hits, "viewcos_limit", view_cos, lim)
    if view_cos < lim:
        _hit(hits, "viewcos_low")
        return False
    mp.level = _level(frame, mp, dist, hits)
    mp.track_in_view = True
    mp.proj_x, mp.proj_y, mp.view_cos = u, v, view_cos
    return True


# ---------------------------------------------------------------- (a) SearchLocalPoints
def search_local_points(frame, local_points, query_seen=None, th=1.0, nnratio=0.8, viewing_cos_limit=0.5, rules=REFERENCE, hits=None):
    """Tracking::SearchLocalPoints from its first loop to the matcher's return; frame.slots are mCurrentFrame.mvpMapPoints on
    entry and are changed as the reference changes them.  query_seen[q]: mnLastFrameSeen of local point q already equals this
    frame's id (Tracking.cc:781, :904).  Returns a dict of what pgorb_search_local_points reports, plus `front`: the arrays
    pgorb_search_by_projection_points takes."""
    for q, mp in enumerate(local_points):
        mp.last_frame_seen = frame.id if (query_seen is not None and query_seen[q]) else -1
        mp.track_in_view = False
    entry_bad = {i for i, mp in enumerate(frame.slots) if mp is not None and mp.bad}
    for i, mp in enumerate(frame.slots):                                       # :1137-1153
        if mp is None:
            continue
        if mp.bad:
            _hit(hits, "slot_bad")
            if rules.bad_slot == "cleared":
                frame.slots[i] = None
        else:
            _hit(hits, "slot_seen")
            mp.last_frame_seen = frame.id
            mp.track_in_view = False
    n_to_match = 0
    for q, mp in enumerate(local_points):                                      # :1158-1171
        if mp.last_frame_seen == frame.id:
            _hit(hits, "query_seen_flag" if (query_seen is not None and query_seen[q]) else "query_in_slot")
            if rules.seen == "skipped":
                continue
        if mp.bad:
            _hit(hits, "query_bad")
            continue
        if is_in_frustum(frame, mp, viewing_cos_limit, rules, hits):
            n_to_match += 1
    nq, n = len(local_points), len(frame.keys)
    in_view = np.array([mp.track_in_view for mp in local_points], np.uint8).reshape(nq)
    z = lambda dt: np.zeros(nq, dt)
    px, py, lv, vc = z(np.float32), z(np.float32), z(np.int32), z(np.float32)
    for q, mp in enumerate(local_points):
        if mp.track_in_view:
            px[q], py[q], lv[q], vc[q] = mp.proj_x, mp.proj_y, mp.level, mp.view_cos
    kp_out = np.array([-1 if s is None else s.id for s in frame.slots], np.int32).reshape(n)
    has = np.array([1 if (s is not None and s.has_obs) else 0 for s in frame.slots], np.uint8).reshape(n)
    if n_to_match == 0:
        _hit(hits, "n_to_match_zero")
    # SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:46-131); skipped when nToMatch == 0 (the same result)
    assigned = [-1] * n
    nmatches = 0
    thf = f32(th)
    factor = thf != f32(1.0)
    for q, mp in enumerate(local_points):
        if not mp.track_in_view or mp.bad:
            continue
        lvl = mp.level
        r = R.radius_by_viewing_cos(mp.view_cos)
        _hit(hits, "viewcos_above_0998" if float(mp.view_cos) > 0.998 else "viewcos_below_0998")
        if factor:
            r = f32(r * thf)
        cand = frame.grid.features_in_area(mp.proj_x, mp.proj_y, f32(r * frame.sf[lvl]), lvl - 1, lvl, hits)
        if not cand:
            continue
        best, best_level, best2, best_level2, best_idx = 256, -1, 256, -1, -1
        for i in cand:
            s = frame.slots[i]
            if s is not None and s.has_obs:                                   # Observations() > 0 (:79-81)
                _hit(hits, "candidate_blocked")
                continue
            d = _dist(mp.dint, frame.dint[i])
            if d < best:
                best2, best = best, d
                best_level2, best_level = best_level, int(frame.keys["octave"][i])
                best_idx = i
            elif d < best2:
                best_level2, best2 = int(frame.keys["octave"][i]), d
        if best <= TH_HIGH:
            if best_level == best_level2 and R._ratio_gt(best, nnratio, best2, R.REFERENCE):
                continue
            if best_idx in entry_bad:
                _hit(hits, "bad_slot_keypoint_taken")
            frame.slots[best_idx] = mp
            assigned[best_idx] = q
            nmatches += 1
    front = dict(kp_has_point=has, valid=in_view.copy(), proj_x=px, proj_y=py, level=lv, view_cos=vc,
                 pdesc=np.array([mp.desc for mp in local_points], np.uint8).reshape(nq, 32),
                 pobs=np.array([mp.has_obs for mp in local_points], np.uint8).reshape(nq))
    return dict(nmatches=nmatches, assigned=np.array(assigned, np.int32).reshape(n), in_view=in_view, proj_x=px, proj_y=py, level=lv,
                view_cos=vc, kp_point_out=kp_out, n_to_match=n_to_match, front=front)


# ---------------------------------------------------------------- (b), (c): the two frame-to-frame forms
def _best_only(frame, blocked, dq, u, v, radius, lvl, th_take, angle, hist, assigned, q, check_orientation, hits):
    """The descriptor loop both forms share (:1404-1440 / :1542-1572): best distance only, first minimum wins."""
    cand = frame.grid.features_in_area(u, v, radius, lvl - 1, lvl + 1, hits)
    if not cand:
        return None
    best, best_idx = 256, -1
    for i in cand:
        if blocked[i]:
            _hit(hits, "candidate_blocked")
            continue
        d = _dist(dq, frame.dint[i])
        if d < best:
            best, best_idx = d, i
    if best <= th_take:
        assigned[best_idx] = q
        if check_orientation:
            hist[R.rotation_bin(angle, frame.keys["angle"][best_idx], R.REFERENCE, hits)].append(best_idx)
        return best_idx
    return None


def _finish(hist, assigned, nmatches, check_orientation, hits):
    if check_orientation:
        for b in R._drop_outside_three_maxima(hist, R.REFERENCE, hits):
            for i in hist[b]:
                assigned[i] = -1
                nmatches -= 1
    return nmatches


def search_by_projection_last_frame(frame, last_keys, last_points, last_outlier=None, kp_has_point=None, th=15.0, check_orientation=True,
                                    rules=REFERENCE, hits=None):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono = true): query i is the last frame's keypoint i.  kp_has_point[i]:
    CurrentFrame.mvpMapPoints[i] holds a point with Observations() > 0 on entry.  Returns a dict of what
    pgorb_search_by_projection_last_frame reports, plus `front`: the arrays pgorb_search_by_projection_frame takes."""
    n, nl = len(frame.keys), len(last_keys)
    blocked = [bool(kp_has_point[i]) if kp_has_point is not None else False for i in range(n)]
    assigned = [-1] * n
    hist = [[] for _ in range(HISTO_LENGTH)]
    valid, us, vs = np.zeros(nl, np.uint8), np.zeros(nl, np.float32), np.zeros(nl, np.float32)
    nmatches = 0
    for i in range(nl):
        mp = last_points[i]
        if mp is None:
            _hit(hits, "last_null")
            continue
        if last_outlier is not None and last_outlier[i]:
            _hit(hits, "last_outlier")
            continue
        if mp.bad:
            _hit(hits, "last_bad")
            if rules.last_frame_bad_skip == "on":
                continue
        pc = to_camera(frame.pose, mp.pos, rules)
        _z_hits(hits, pc[2])
        with np.errstate(all="ignore"):
            invzc = f32(1.0 / f64(pc[2]))                                    # const float invzc = 1.0/x3Dc.at<float>(2)
        if invzc < 0:
            _hit(hits, "invz_negative")
            continue
        u, v = project(frame.pose, pc, invzc)
        if not in_bounds(frame, u, v, rules, hits):
            continue
        octave = int(last_keys["octave"][i])
        valid[i], us[i], vs[i] = 1, u, v
        radius = f32(f32(th) * frame.sf[octave])
        got = _best_only(frame, blocked, mp.dint, u, v, radius, octave, TH_HIGH, last_keys["angle"][i], hist, assigned, i,
                         check_orientation, hits)
        if got is not None:
            if mp.bad:
                _hit(hits, "last_bad_matched")
            blocked[got] = mp.has_obs
            nmatches += 1
    nmatches = _finish(hist, assigned, nmatches, check_orientation, hits)
    pts = [mp for mp in last_points]
    front = dict(valid=valid.copy(), u=us, v=vs, last_octave=np.asarray(last_keys["octave"], np.int32), last_angle=np.asarray(last_keys["angle"], np.float32),
                 pdesc=np.array([np.zeros(32, np.uint8) if mp is None else mp.desc for mp in pts], np.uint8).reshape(nl, 32),
                 pobs=np.array([0 if mp is None else mp.has_obs for mp in pts], np.uint8).reshape(nl))
    return dict(nmatches=nmatches, assigned=np.array(assigned, np.int32).reshape(n), valid=valid, u=us, v=vs, front=front)


def search_by_projection_keyframe(frame, kf_keys, kf_points, already_found=None, kp_has_point=None, th=10.0, orb_dist=100,
                                  check_orientation=True, rules=REFERENCE, hits=None):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): query i is the key frame's keypoint i; any point in
    CurrentFrame.mvpMapPoints[i] blocks (kp_has_point).  Returns a dict of what pgorb_search_by_projection_keyframe_pose reports,
    plus `front`: the arrays pgorb_search_by_projection_keyframe takes."""
    n, nk = len(frame.keys), len(kf_keys)
    held = [bool(kp_has_point[i]) if kp_has_point is not None else False for i in range(n)]
    assigned = [-1] * n
    hist = [[] for _ in range(HISTO_LENGTH)]
    z = lambda: np.zeros(nk, np.float32)
    us, vs, d3s, mind, maxd = z(), z(), z(), z(), z()
    valid = np.zeros(nk, np.uint8)
    nmatches = 0
    for i in range(nk):
        mp = kf_points[i]
        if mp is None:
            _hit(hits, "kf_null")
            continue
        if mp.bad:
            _hit(hits, "kf_bad")
            continue
        if already_found is not None and already_found[i]:
            _hit(hits, "kf_found")
            continue
        pc = to_camera(frame.pose, mp.pos, rules)
        _z_hits(hits, pc[2])
        with np.errstate(all="ignore"):
            invzc = f32(1.0 / f64(pc[2]))
        if rules.reloc_depth_sign == "on" and invzc < 0:
            continue
        u, v = project(frame.pose, pc, invzc)
        if not in_bounds(frame, u, v, rules, hits):
            continue
        _, dist3d = dist_to_centre(frame.pose, mp.pos, rules)
        valid[i], us[i], vs[i], d3s[i], mind[i], maxd[i] = 1, u, v, dist3d, mp.min_d, mp.max_d
        if not _depth_ok(mp, dist3d, hits):
            continue
        lvl = _level(frame, mp, dist3d, hits)
        radius = f32(f32(th) * frame.sf[lvl])
        got = _best_only(frame, held, mp.dint, u, v, radius, lvl, orb_dist, kf_keys["angle"][i], hist, assigned, i, check_orientation, hits)
        if got is not None:
            if pc[2] < 0:
                _hit(hits, "behind_camera_matched")
            held[got] = True
            nmatches += 1
    nmatches = _finish(hist, assigned, nmatches, check_orientation, hits)
    front = dict(valid=valid.copy(), found=np.zeros(nk, np.uint8), u=us, v=vs, dist3d=d3s, min_distance=mind, max_distance=maxd,
                 kf_angle=np.asarray(kf_keys["angle"], np.float32),
                 pdesc=np.array([np.zeros(32, np.uint8) if mp is None else mp.desc for mp in kf_points], np.uint8).reshape(nk, 32))
    return dict(nmatches=nmatches, assigned=np.array(assigned, np.int32).reshape(n), u=us, v=vs, dist3d=d3s, front=front)
