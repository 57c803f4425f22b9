"""A plain, sequential restatement of loop closing's four matchers (thirdparty/orb-slam2/src/ORBmatcher.cc), monocular -- the two
Scw matchers first, then search_by_sim3 (:1106-1330) and search_by_bow_keyframes (:524-657) further down:
    search_by_projection_sim3   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)    :292-405
    fuse_sim3                   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)              :981-1104
with KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:672-716) and GetMapPoints (:338-351).  Written from that upstream text
and the cv::Mat readings of DESIGN.md section 4; it goes through objects query by query, does not use oracle/, and shares no
code with the mirror (pilotguru_amd/orb.py) or the kernels (pilotguru_amd/csrc/loop.hip).  The objects are fuse_reference's
KeyFrame and MapPoint; the key frame's pose record holds the DECOMPOSED Scw (Rcw | tcw, Ow), as the ABI takes it.

`rules` (a Rules) switches one decision at a time, `hits` (a collections.Counter or None) counts the edges reached.  The
two-pass functions at the end are the kernels' specification.
"""
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_reference as MR  # noqa: E402
from fuse_reference import _LOG_F  # noqa: E402
from matcher_reference import TH_LOW, _dist, _hit, predict_scale  # noqa: E402

f32, f64 = np.float32, np.float64
SKIPPED, NO_MATCH, ADDED, KF_POINT_BAD, REPLACE_REQUESTED = 0, 1, 2, 5, 6      # PGORB_FUSE_* (include/pgorb.h)


@dataclass(frozen=True)
class Rules:
    found: str = "entry"         # 3: spAlreadyFound is the set on entry (:308) | "live": a match written by this call joins it
    taken: str = "skip"          # 3: a candidate whose vpMatched[idx] is set is skipped (:377) | "ignore"
    angle: str = "double"        # PO.dot(Pn) < 0.5*dist in double | "float" | "off": no viewing-angle test
    levels: str = "l"            # octave in [level - 1, level] | "l+1"
    max_bound: str = "strict"    # IsInImage: x < mnMaxX | "inclusive"
    th_low: str = "le"           # bestDist <= TH_LOW | "lt"
    tie: str = "first"           # dist < bestDist | "last": <=
    chi2: str = "off"            # 4: no chi-square test | "on": Fuse(pKF, points)'s (:941-948)
    bad_occ: str = "count"       # 4: a bad occupant still counts toward nFused (:1099) | "skip"
    later: str = "replace"       # 4: a later query on a slot this call filled sees its occupant (:1088-1093) | "added"
    already: str = "on"          # 4: points already in the key frame are skipped (:1009) | "off"


REFERENCE = Rules()
MUTANTS = {
    "found=live": Rules(found="live"),
    "taken=ignore": Rules(taken="ignore"),
    "angle=off": Rules(angle="off"),
    "angle=float": Rules(angle="float"),
    "levels=l+1": Rules(levels="l+1"),
    "max_bound=inclusive": Rules(max_bound="inclusive"),
    "th_low=lt": Rules(th_low="lt"),
    "tie=last": Rules(tie="last"),
    "chi2=on": Rules(chi2="on"),
    "bad_occ=skip": Rules(bad_occ="skip"),
    "later=added": Rules(later="added"),
    "already=off": Rules(already="off"),
}
# which routine a mutant changes (both: every rule of the shared front part)
ONLY_3 = {"found=live", "taken=ignore"}
ONLY_4 = {"chi2=on", "bad_occ=skip", "later=added", "already=off"}


def front(kf, mp, th, rules=REFERENCE, hits=None):
    """:322-367 / :1012-1058 for one point that is neither bad nor already found: None where the reference `continue`s, else
    (u, v, level, vIndices) with vIndices non-empty."""
    T = np.asarray(kf.pose["Tcw"], np.float32).reshape(3, 4)
    Ow = np.asarray(kf.pose["Ow"], np.float32).reshape(3)
    fx, fy, cx, cy = (f32(kf.pose[k]) for k in ("fx", "fy", "cx", "cy"))
    p = mp.pos
    # p3Dc = Rcw*p3Dw + tcw: gemm's small-matrix path, tcw as gemm's C
    pc = [f32(f64(MR.gemm3(T[r][0], T[r][1], T[r][2], p[0], p[1], p[2])) + f64(T[r][3])) for r in range(3)]
    if pc[2] < f32(0):
        _hit(hits, "behind")
        return None
    with np.errstate(all="ignore"):
        invz = f32(f32(1) / pc[2])
        u, v = f32(f32(fx * f32(pc[0] * invz)) + cx), f32(f32(fy * f32(pc[1] * invz)) + cy)
    if u == kf.ibounds[1] or v == kf.ibounds[3]:
        _hit(hits, "on_max_bound")
    mnx, mxx, mny, mxy = kf.ibounds
    inside = (u >= mnx and u <= mxx and v >= mny and v <= mxy) if rules.max_bound == "inclusive" else \
        (u >= mnx and u < mxx and v >= mny and v < mxy)
    if not inside:
        _hit(hits, "outside_image")
        return None
    max_d, min_d = f32(f32(1.2) * mp.max_d), f32(f32(0.8) * mp.min_d)            # Get{Max,Min}DistanceInvariance
    PO = [f32(p[i] - Ow[i]) for i in range(3)]
    dist = f32(MR.normd(PO, MR.Rules()))
    if dist == min_d:
        _hit(hits, "on_depth_min")
    if dist == max_d:
        _hit(hits, "on_depth_max")
    if dist < min_d or dist > max_d:
        _hit(hits, "depth_low" if dist < min_d else "depth_high")
        return None
    if rules.angle != "off":
        dot = MR.dotd(PO, mp.normal, MR.Rules(norm="float" if rules.angle == "float" else "double"))
        if dot < 0.5 * f64(dist):
            _hit(hits, "angle")
            return None
    level = predict_scale(mp.max_d, dist, kf.log_sf, kf.nlevels, _LOG_F())
    radius = f32(f32(th) * f32(kf.sf[level]))
    idxs = kf.features_in_area(u, v, radius)
    if not idxs:
        _hit(hits, "no_candidate")
        return None
    return u, v, level, idxs


def best_of(kf, mp, u, v, level, idxs, rules, hits, skip=None):
    """The descriptor loop (:372-394 / :1064-1083): (bestDist, bestIdx), 256 / -1 when nothing passes."""
    dmp = int.from_bytes(mp.desc.tobytes(), "little")
    best_dist, best_idx = 256, -1
    hi = level + 1 if rules.levels == "l+1" else level
    for idx in idxs:
        if skip is not None and skip(idx):
            _hit(hits, "taken_skipped")
            continue
        kp = kf.keys[idx]
        o = int(kp["octave"])
        if o == level + 1:
            _hit(hits, "octave_above")
        if o < level - 1 or o > hi:
            continue
        if rules.chi2 == "on":
            ex, ey = f32(u - f32(kp["x"])), f32(v - f32(kp["y"]))
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            if float(f32(e2 * f32(kf.inv_sigma2[o]))) > 5.99:
                continue
        dist = _dist(dmp, kf.dint[idx])
        if dist == best_dist:
            _hit(hits, "tie")
        if dist < best_dist or (rules.tie == "last" and dist == best_dist):
            best_dist, best_idx = dist, idx
    if best_dist in (TH_LOW, TH_LOW + 1):
        _hit(hits, "dist_%d" % best_dist)
    return best_dist, best_idx


def _accept(d, rules):
    return d < TH_LOW if rules.th_low == "lt" else d <= TH_LOW


def search_by_projection_sim3(kf, points, matched, th, rules=REFERENCE, hits=None):
    """:292-405.  `matched` (a list of MapPoint or None, one per keypoint) is vpMatched and is changed in place.  Returns
    (nmatches, assigned) with assigned[i] = the query index whose point this call wrote into matched[i], or -1."""
    already = {id(m) for m in matched if m is not None}                       # :308-309
    assigned = [-1] * len(matched)
    nmatches = 0
    for q, mp in enumerate(points):
        if mp.bad:
            _hit(hits, "bad")
            continue
        if id(mp) in already:
            _hit(hits, "already_found")
            continue
        fr = front(kf, mp, th, rules, hits)
        if fr is None:
            continue
        u, v, level, idxs = fr
        skip = (lambda i: matched[i] is not None) if rules.taken == "skip" else None
        bd, bi = best_of(kf, mp, u, v, level, idxs, rules, hits, skip)
        if _accept(bd, rules):
            if assigned[bi] >= 0 or matched[bi] is not None:
                _hit(hits, "overwrote")                                       # (only without the :377 skip)
            matched[bi] = mp
            assigned[bi] = q
            nmatches += 1
            _hit(hits, "matched")
            if rules.found == "live":
                already.add(id(mp))
        else:
            _hit(hits, "no_match")
    return nmatches, assigned


def fuse_sim3(kf, points, th, rules=REFERENCE, hits=None):
    """:981-1104.  kf.slots is mvpMapPoints and is changed in place (AddMapPoint).  Returns (nFused, [(action, replace point or
    None, bestIdx, bestDist)])."""
    already = {id(s) for s in kf.slots if s is not None and not s.bad}        # GetMapPoints() (KeyFrame.cc:338-351)
    nfused, out = 0, []
    for mp in points:
        if mp.bad:
            _hit(hits, "bad")
            out.append((SKIPPED, None, -1, -1))
            continue
        if id(mp) in already and rules.already == "on":
            _hit(hits, "already_found")
            out.append((SKIPPED, None, -1, -1))
            continue
        fr = front(kf, mp, th, rules, hits)
        if fr is None:
            out.append((SKIPPED, None, -1, -1))
            continue
        u, v, level, idxs = fr
        bd, bi = best_of(kf, mp, u, v, level, idxs, rules, hits)
        if not _accept(bd, rules):
            _hit(hits, "no_match")
            out.append((NO_MATCH, None, bi, bd))
            continue
        occ = kf.slots[bi]
        if occ is not None and rules.later == "added" and getattr(occ, "_added_by_call", False):
            occ = None
        if occ is not None:
            if not occ.bad:
                _hit(hits, "replace_self" if occ is mp else "replace_requested")
                out.append((REPLACE_REQUESTED, occ, bi, bd))
            else:
                _hit(hits, "kf_point_bad")
                if rules.bad_occ == "skip":
                    out.append((SKIPPED, None, bi, bd))
                    continue
                out.append((KF_POINT_BAD, None, bi, bd))
        else:
            _hit(hits, "added")
            kf.slots[bi] = mp                                                 # AddObservation + AddMapPoint
            mp._added_by_call = True
            out.append((ADDED, None, bi, bd))
        nfused += 1
    return nfused, out


# ---------------------------------------------------------------- the two-pass forms (the kernels' specification)
def search_by_projection_two_pass(kf, points, matched, th):
    """pgorb_search_by_projection_sim3's decomposition.  Pass 1, every query on its own, from the entry state: its candidates
    that are unmatched on entry and pass the octave test, in scan order, WITHOUT those of distance above TH_LOW.  Pass 2, the
    queries in order: the smallest-distance untaken entry (first in scan order among equals) is taken.
    Why dropping is exact: the reference takes bestIdx only if bestDist <= TH_LOW, and bestDist is the minimum over the untaken
    candidates; if that minimum is <= TH_LOW it is attained inside the shortened list (same first-in-order winner), and if it is
    above, the shortened list has no untaken entry and the query takes nothing -- in both cases the same decision, and decisions
    are all that later queries see."""
    already = {id(m) for m in matched if m is not None}
    lists = []
    for mp in points:                                                         # pass 1: no query depends on another
        lst = []
        if not mp.bad and id(mp) not in already:
            fr = front(kf, mp, th)
            if fr is not None:
                u, v, level, idxs = fr
                dmp = int.from_bytes(mp.desc.tobytes(), "little")
                for idx in idxs:
                    o = int(kf.keys[idx]["octave"])
                    if matched[idx] is not None or o < level - 1 or o > level:
                        continue
                    d = _dist(dmp, kf.dint[idx])
                    if d <= TH_LOW:
                        lst.append((d, len(lst), idx))
        lists.append(lst)
    taken = [m is not None for m in matched]
    out = list(matched)
    assigned = [-1] * len(matched)
    n = 0
    for q, lst in enumerate(lists):                                           # pass 2
        free = [e for e in lst if not taken[e[2]]]
        if free:
            idx = min(free)[2]
            taken[idx] = True
            out[idx] = points[q]
            assigned[idx] = q
            n += 1
    return n, assigned, out


def fuse_two_pass(kf, points, th):
    """pgorb_fuse_sim3's decomposition: every query matched from the entry state (matching never reads the slots), then per slot
    the first matched query in list order finds an empty slot empty and is ADDED, every later one sees that query's point.
    Changes nothing; returns (nFused, [(action, replace point or None, bestIdx, bestDist)], slots afterwards)."""
    already = {id(s) for s in kf.slots if s is not None and not s.bad}
    first = []
    for mp in points:
        r = (SKIPPED, -1, -1)
        if not mp.bad and id(mp) not in already:
            fr = front(kf, mp, th)
            if fr is not None:
                bd, bi = best_of(kf, mp, *fr, REFERENCE, None)
                r = (ADDED if bd <= TH_LOW else NO_MATCH, bi, bd)
        first.append(r)
    winner = {}
    for q, (a, bi, _) in enumerate(first):                                    # atomicMin of the query index per slot
        if a == ADDED and bi not in winner:
            winner[bi] = q
    slots = list(kf.slots)
    out, nf = [], 0
    for q, (a, bi, bd) in enumerate(first):
        if a != ADDED:
            out.append((a, None, bi, bd))
            continue
        nf += 1
        occ = kf.slots[bi]
        if occ is not None:
            out.append((KF_POINT_BAD, None, bi, bd) if occ.bad else (REPLACE_REQUESTED, occ, bi, bd))
        elif winner[bi] == q:
            slots[bi] = points[q]
            out.append((ADDED, None, bi, bd))
        else:
            out.append((REPLACE_REQUESTED, points[winner[bi]], bi, bd))
    return nf, out, slots


def decide_in_rounds(lists, taken):
    """Pass 2 of search_by_projection_two_pass without its sequence, as k_ps3_decide runs it.  lists[q] = [(distance, position,
    keypoint)], taken = the entry state.  Per round minq[i] = the smallest undecided query listing the untaken keypoint i; a query
    is ready when minq[i] is itself for every untaken i of its list; the ready ones decide from the state as it is, then all
    apply.  Returns ({keypoint: query}, number of rounds)."""
    taken = list(taken)
    pending = [q for q, lst in enumerate(lists) if lst]
    assigned, rounds = {}, 0
    while pending:
        rounds += 1
        minq = {}
        for q in pending:
            for _, _, i in lists[q]:
                if not taken[i]:
                    minq[i] = min(minq.get(i, q), q)
        decided, nxt = [], []
        for q in pending:
            free = [e for e in lists[q] if not taken[e[2]]]
            if all(minq[e[2]] == q for e in free):
                decided.append((q, min(free)[2] if free else -1))
            else:
                nxt.append(q)
        assert decided and decided[0][0] == pending[0]                       # the smallest undecided query is always ready
        for q, i in decided:
            if i >= 0:
                assert not taken[i]
                taken[i] = True
                assigned[i] = q
        pending = nxt
    return assigned, rounds


# ---------------------------------------------------------------- SearchBySim3 (ORBmatcher.cc:1106-1330)
TH_HIGH = 100


@dataclass(frozen=True)
class Rules2:
    cam: str = "kf1"             # both projections use pKF1's fx, fy, cx, cy (:1109-1112) | "own": the first one uses pKF2's
    norm: str = "cam"            # dist3D = cv::norm(p3Dc) of the camera-frame vector (:1183) | "world": norm(p3Dw - Ow)
    th: str = "high"             # bestDist <= TH_HIGH (:1225) | "low": TH_LOW
    agree: str = "on"            # vnMatch2[vnMatch1[i1]] == i1 (:1321) | "off": every vnMatch1 counts
    already2: str = "on"         # vbAlreadyMatched2 slots are not projected (:1236) | "off"
    levels: str = "l"            # octave in [level - 1, level] | "l+1"
    max_bound: str = "strict"    # IsInImage: x < mnMaxX | "inclusive"
    tie: str = "first"           # dist < bestDist | "last"


REFERENCE2 = Rules2()
MUTANTS2 = {
    "cam=own": Rules2(cam="own"),
    "norm=world": Rules2(norm="world"),
    "th=low": Rules2(th="low"),
    "agree=off": Rules2(agree="off"),
    "already2=off": Rules2(already2="off"),
    "levels=l+1": Rules2(levels="l+1"),
    "tie=last": Rules2(tie="last"),
}
# Rules2(max_bound="inclusive") is NOT in the table: no pair case here puts a projection exactly on mnMaxX, so nothing separates it
# in SearchBySim3.  The strict bound is pinned by the u_on_max case of the two Scw routines, which share the kernel-side test.


def _gemm_c(M, x, c):
    """M*x + c on gemm's small-matrix path: float sums of three products, then + c in double, rounded to float."""
    return [f32(f64(MR.gemm3(M[r][0], M[r][1], M[r][2], x[0], x[1], x[2])) + f64(c[r])) for r in range(3)]


def _sim3_direction(src, dst, cam, sR, t, already, th, rules, hits, first):
    """One of the two loops (:1152-1229 / :1232-1309): vnMatch of every slot of `src` projected into `dst` with camera `cam`."""
    T = np.asarray(src.pose["Tcw"], np.float32).reshape(3, 4)
    sR = np.asarray(sR, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    out = [-1] * len(src.slots)
    for i, mp in enumerate(src.slots):
        if mp is None:
            continue
        if already[i]:
            _hit(hits, "already%d" % (1 if first else 2))
            continue
        if mp.bad:
            _hit(hits, "bad")
            continue
        pc = _gemm_c(T[:, :3], mp.pos, T[:, 3])
        pt = _gemm_c(sR, pc, t)
        if pt[2] < f32(0):
            _hit(hits, "behind")
            continue
        with np.errstate(all="ignore"):
            invz = f32(1.0 / f64(pt[2]))
            u, v = f32(f32(fx * f32(pt[0] * invz)) + cx), f32(f32(fy * f32(pt[1] * invz)) + cy)
        mnx, mxx, mny, mxy = dst.ibounds
        inside = (u >= mnx and u <= mxx and v >= mny and v <= mxy) if rules.max_bound == "inclusive" else \
            (u >= mnx and u < mxx and v >= mny and v < mxy)
        if not inside:
            _hit(hits, "outside_image")
            continue
        if rules.norm == "world":
            Ow = np.asarray(dst.pose["Ow"], np.float32)
            dist = f32(MR.normd([f32(mp.pos[k] - Ow[k]) for k in range(3)], MR.Rules()))
        else:
            dist = f32(MR.normd(pt, MR.Rules()))
        if dist < f32(f32(0.8) * mp.min_d) or dist > f32(f32(1.2) * mp.max_d):
            _hit(hits, "depth")
            continue
        level = predict_scale(mp.max_d, dist, dst.log_sf, dst.nlevels, _LOG_F())
        idxs = dst.features_in_area(u, v, f32(f32(th) * f32(dst.sf[level])))
        if not idxs:
            _hit(hits, "no_candidate")
            continue
        dmp = int.from_bytes(mp.desc.tobytes(), "little")
        best_dist, best_idx = 2 ** 31 - 1, -1
        hi = level + 1 if rules.levels == "l+1" else level
        for idx in idxs:
            o = int(dst.keys[idx]["octave"])
            if o < level - 1 or o > hi:
                continue
            d = _dist(dmp, dst.dint[idx])
            if d == best_dist:
                _hit(hits, "tie")
            if d < best_dist or (rules.tie == "last" and d == best_dist):
                best_dist, best_idx = d, idx
        if TH_LOW < best_dist <= TH_HIGH:
            _hit(hits, "between_thresholds")
        if best_dist <= (TH_LOW if rules.th == "low" else TH_HIGH):
            out[i] = best_idx
    return out


def search_by_sim3(kf1, kf2, sim3, already1, already2, th, rules=REFERENCE2, hits=None):
    """:1106-1330.  kf1 / kf2: KeyFrames whose slots hold MapPoints; sim3: a record with sR12, t12, sR21, t21.  Returns
    (nFound, match12) with match12[i1] = idx2 of every newly found pair or -1."""
    a2 = already2 if rules.already2 == "on" else [False] * len(kf2.slots)
    m1 = _sim3_direction(kf1, kf2, kf2.pose if rules.cam == "own" else kf1.pose, sim3["sR21"], sim3["t21"], already1, th, rules, hits, True)
    m2 = _sim3_direction(kf2, kf1, kf1.pose, sim3["sR12"], sim3["t12"], a2, th, rules, hits, False)
    match12, n = [-1] * len(kf1.slots), 0
    for i1, idx2 in enumerate(m1):
        if idx2 >= 0:
            if m2[idx2] == i1 or rules.agree == "off":
                match12[i1] = idx2
                n += 1
            else:
                _hit(hits, "disagree")
    return n, match12


# ---------------------------------------------------------------- SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:524-657)
@dataclass(frozen=True)
class Rules1:
    th_low: str = "lt"           # bestDist1 < TH_LOW (:600) | "le": SearchByBoW(KeyFrame*, Frame&)'s <=
    matched2: str = "on"         # a KF2 keypoint matched by this call is skipped (:578) | "off"
    valid2: str = "on"           # a KF2 keypoint without a (good) map point is skipped (:578-582) | "off"
    valid1: str = "on"           # a KF1 keypoint without a (good) map point is skipped (:560-564) | "off"
    ratio: str = "on"            # (float)bestDist1 < mfNNratio*(float)bestDist2 (:602) | "off"


REFERENCE1 = Rules1()
MUTANTS1 = {"th_low=le": Rules1(th_low="le"), "matched2=off": Rules1(matched2="off"), "valid2=off": Rules1(valid2="off"),
            "valid1=off": Rules1(valid1="off"), "ratio=off": Rules1(ratio="off")}


def search_by_bow_keyframes(desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2, nnratio, check_orientation=True,
                            rules=REFERENCE1, hits=None):
    """Returns (nmatches, matches12) with matches12[idx1] = the KF2 keypoint whose map point goes to vpMatches12[idx1], or -1."""
    import bisect
    from matcher_reference import HISTO_LENGTH, _drop_outside_three_maxima, _ratio_lt, descriptor_ints, rotation_bin
    from matcher_reference import REFERENCE as MREF
    d1, d2 = descriptor_ints(desc1), descriptor_ints(desc2)
    nodes1, start1, feat1 = [[int(x) for x in a] for a in fv1]
    nodes2, start2, feat2 = [[int(x) for x in a] for a in fv2]
    matches12 = [-1] * len(d1)
    matched2 = [False] * len(d2)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    a = b = 0
    while a < len(nodes1) and b < len(nodes2):
        if nodes1[a] == nodes2[b]:
            _hit(hits, "common_node")
            if start1[a + 1] - start1[a] > 64 and start2[b + 1] - start2[b] > 64:
                _hit(hits, "big_node")
            for idx1 in feat1[start1[a]:start1[a + 1]]:
                if not valid1[idx1] and rules.valid1 == "on":
                    _hit(hits, "invalid1")
                    continue
                best1, best_idx2, best2 = 256, -1, 256
                for idx2 in feat2[start2[b]:start2[b + 1]]:
                    if matched2[idx2] and rules.matched2 == "on":
                        _hit(hits, "matched2_skipped")
                        continue
                    if not valid2[idx2] and rules.valid2 == "on":
                        _hit(hits, "invalid2")
                        continue
                    d = _dist(d1[idx1], d2[idx2])
                    if d < best1:
                        best2, best1, best_idx2 = best1, d, idx2
                    elif d < best2:
                        best2 = d
                if best1 == TH_LOW:
                    _hit(hits, "dist_50")
                if best1 < TH_LOW or (rules.th_low == "le" and best1 == TH_LOW):
                    if rules.ratio == "off" or _ratio_lt(best1, nnratio, best2, MREF):
                        matches12[idx1] = best_idx2
                        matched2[best_idx2] = True
                        if check_orientation:
                            hist[rotation_bin(angle1[idx1], angle2[best_idx2])].append(idx1)
                        nmatches += 1
                    else:
                        _hit(hits, "ratio_failed")
            a += 1
            b += 1
        elif nodes1[a] < nodes2[b]:
            a = bisect.bisect_left(nodes1, nodes2[b])
        else:
            b = bisect.bisect_left(nodes2, nodes1[a])
    if check_orientation:
        for bn in _drop_outside_three_maxima(hist, MREF, None):
            for i in hist[bn]:
                _hit(hits, "rotation_dropped")
                matches12[i] = -1
                nmatches -= 1
    return nmatches, matches12
