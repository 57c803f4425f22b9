"""A plain, sequential restatement of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (thirdparty/orb-slam2/src/
ORBmatcher.cc:827-979), monocular, with the MapPoint and KeyFrame members it calls -- Observations / AddObservation (MapPoint.cc:
100-130), Replace (:196-232), ComputeDistinctiveDescriptors (:257-318), IsInKeyFrame (:402-406), GetFeaturesInArea / IsInImage
(KeyFrame.cc:672-716) -- and LocalMapping::SearchInNeighbors' two rounds of it (LocalMapping.cc:487-516).  It is written from that
upstream text and the cv::Mat readings of DESIGN.md section 4 (the helpers of tests/mapping_reference.py); it does not use oracle/
and was not derived from the HIP kernels (pilotguru_amd/csrc/fuse.hip).

Objects are real: a MapPoint holds an observation dict {KeyFrame: index} and a bad flag, a KeyFrame holds its slots.  Key frames
are ordered by mnId where the reference iterates a std::map<KeyFrame*, size_t> (by address).  `rules` (a Rules) switches one
reading or rule at a time; `hits` (a collections.Counter or None) counts the edges reached.
"""
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapping_reference as MR  # noqa: E402
from matcher_reference import GRID_COLS, GRID_ROWS, TH_LOW, Grid, _dist, _hit, predict_scale  # noqa: E402

f32, f64 = np.float32, np.float64
SKIPPED, NO_MATCH, ADDED, MERGED, REPLACED, KF_POINT_BAD = range(6)      # PGORB_FUSE_* (include/pgorb.h)


@dataclass(frozen=True)
class Rules:
    gemm: str = "float"          # Rcw*p3Dw + tcw on gemm's small-matrix path (float sums) | "double"
    norm: str = "double"         # cv::norm(PO) in double | "float"
    dot: str = "double"          # PO.dot(Pn) in double | "float"
    tie: str = "first"           # dist < bestDist: the first candidate in scan order wins a tie | "last": <=
    th_low: str = "le"           # bestDist <= TH_LOW fuses | "lt"
    obs_cmp: str = "gt"          # pMPinKF->Observations() > pMP->Observations() keeps the occupant | "ge"
    levels: str = "l"            # octave in [level - 1, level] | "l+1": [level - 1, level + 1]
    max_bound: str = "strict"    # IsInImage: x < mnMaxX | "inclusive": x <= mnMaxX
    union: str = "union"         # Replace: the survivor observes the union of both sets | "sum": it counts both lists
    in_kf_skip: str = "on"       # points already in pKF are skipped | "off"


REFERENCE = Rules()
MUTANTS = {
    "gemm=double": Rules(gemm="double"),
    "norm=float": Rules(norm="float"),
    "dot=float": Rules(dot="float"),
    "tie=last": Rules(tie="last"),
    "th_low=lt": Rules(th_low="lt"),
    "obs_cmp=ge": Rules(obs_cmp="ge"),
    "levels=l+1": Rules(levels="l+1"),
    "max_bound=inclusive": Rules(max_bound="inclusive"),
    "union=sum": Rules(union="sum"),
    "in_kf_skip=off": Rules(in_kf_skip="off"),
}


class KeyFrame:
    """The slice of a KeyFrame Fuse reads: mnId, mvKeysUn, mDescriptors, pose, the grid (built from the Frame's float bounds),
    the int bounds it keeps (KeyFrame.h:195-198), the scale tables, and its slots mvpMapPoints."""

    def __init__(self, kf_id, keys, desc, pose, bounds, sf, inv_sigma2, log_sf, nlevels):
        self.id = int(kf_id)
        self.keys = np.ascontiguousarray(keys)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.dint = [int.from_bytes(r.tobytes(), "little") for r in self.desc]
        self.pose = pose
        self.bounds = tuple(float(b) for b in bounds)
        self.grid = Grid(self.keys, self.bounds)
        self.ibounds = tuple(f32(int(f32(b))) for b in bounds)               # const int mnMinX(F.mnMinX) ...
        self.sf, self.inv_sigma2, self.log_sf, self.nlevels = sf, inv_sigma2, log_sf, nlevels
        self.slots = [None] * len(self.keys)
        self.bad = False

    def __lt__(self, other):
        return self.id < other.id

    def is_in_image(self, x, y, rules=REFERENCE):
        mnx, mxx, mny, mxy = self.ibounds
        if rules.max_bound == "inclusive":
            return x >= mnx and x <= mxx and y >= mny and y <= mxy
        return x >= mnx and x < mxx and y >= mny and y < mxy

    def features_in_area(self, x, y, r, hits=None):
        """KeyFrame::GetFeaturesInArea (KeyFrame.cc:672-711): the Frame's grid and cell size, the key frame's int bounds."""
        x, y, r = f32(x), f32(y), f32(r)
        mnx, _, mny, _ = self.ibounds
        g = self.grid
        out = []
        c0 = max(0, int(math.floor(f32(f32(f32(x - mnx) - r) * g.inv_w))))
        if c0 >= GRID_COLS:
            return out
        c1 = min(GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - mnx) + r) * g.inv_w))))
        if c1 < 0:
            return out
        r0 = max(0, int(math.floor(f32(f32(f32(y - mny) - r) * g.inv_h))))
        if r0 >= GRID_ROWS:
            return out
        r1 = min(GRID_ROWS - 1, int(math.ceil(f32(f32(f32(y - mny) + r) * g.inv_h))))
        if r1 < 0:
            return out
        kx, ky = self.keys["x"], self.keys["y"]
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for i in g.cells[ix][iy]:
                    if abs(f32(kx[i] - x)) < r and abs(f32(ky[i] - y)) < r:
                        out.append(i)
        return out


class MapPoint:
    def __init__(self, pid, pos, normal, min_d, max_d, desc):
        self.id = pid
        self.pos = np.asarray(pos, np.float32).reshape(3)
        self.normal = np.asarray(normal, np.float32).reshape(3)
        self.min_d, self.max_d = f32(min_d), f32(max_d)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(32)
        self.obs = {}
        self.nobs = 0
        self.bad = False
        self.replaced = None
        self.found = self.visible = 1

    def observations(self):
        return self.nobs

    def add_observation(self, kf, idx):
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.nobs += 1                                                       # monocular: mvuRight < 0

    def in_kf(self, kf):
        return kf in self.obs

    def replace(self, other, rules=REFERENCE):
        """MapPoint::Replace (MapPoint.cc:196-232)."""
        if other.id == self.id:
            return
        obs = dict(self.obs)
        self.obs.clear()
        self.bad = True
        self.replaced = other
        for kf in sorted(obs):
            idx = obs[kf]
            if not other.in_kf(kf):
                kf.slots[idx] = other                                        # ReplaceMapPointMatch
                other.add_observation(kf, idx)
            else:
                kf.slots[idx] = None                                         # EraseMapPointMatch
                if rules.union == "sum":
                    other.nobs += 1
        other.found += self.found
        other.visible += self.visible
        other.compute_distinctive_descriptors()

    def compute_distinctive_descriptors(self):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:257-318), observations in key-frame id order."""
        if self.bad or not self.obs:
            return
        ds = [kf.desc[self.obs[kf]] for kf in sorted(self.obs) if not kf.bad]
        if not ds:
            return
        di = [int.from_bytes(d.tobytes(), "little") for d in ds]
        n = len(ds)
        best_median, best = 2 ** 31 - 1, 0
        for i in range(n):
            v = sorted(_dist(di[i], di[j]) for j in range(n))
            med = v[int(0.5 * (n - 1))]
            if med < best_median:
                best_median, best = med, i
        self.desc = ds[best].copy()


MATCHED = -3                     # match()'s result for a query with bestDist <= TH_LOW, before its slot is looked at


def match(kf, mp, th=3.0, rules=REFERENCE, hits=None):
    """The part of Fuse's loop body before `pKF->GetMapPoint(bestIdx)` (ORBmatcher.cc:848-962) for one query; changes nothing.
    Returns (SKIPPED, -1, -1), (NO_MATCH, bestIdx, bestDist) or (MATCHED, bestIdx, bestDist)."""
    if mp is None:
        _hit(hits, "null")
        return SKIPPED, -1, -1
    if mp.bad:
        _hit(hits, "bad")
        return SKIPPED, -1, -1
    if mp.in_kf(kf) and rules.in_kf_skip == "on":
        _hit(hits, "in_kf")
        return SKIPPED, -1, -1
    T = np.asarray(kf.pose["Tcw"], np.float32).reshape(3, 4)
    Ow = np.asarray(kf.pose["Ow"], np.float32).reshape(3)
    fx, fy, cx, cy = (f32(kf.pose[k]) for k in ("fx", "fy", "cx", "cy"))
    p = mp.pos
    # p3Dc = Rcw*p3Dw + tcw: gemm's small-matrix path, tcw as gemm's C
    if rules.gemm == "float":
        pc = [f32(f64(MR.gemm3(T[r][0], T[r][1], T[r][2], p[0], p[1], p[2])) + f64(T[r][3])) for r in range(3)]
    else:
        pc = [f32(MR._sumprod(T[r][:3], p) + f64(T[r][3])) for r in range(3)]
    if pc[2] < f32(0):
        _hit(hits, "behind")
        return SKIPPED, -1, -1
    with np.errstate(all="ignore"):
        invz = f32(f32(1) / pc[2])
        x, y = f32(pc[0] * invz), f32(pc[1] * invz)
        u, v = f32(f32(fx * x) + cx), f32(f32(fy * y) + cy)
    if u == kf.ibounds[1] or v == kf.ibounds[3]:
        _hit(hits, "on_max_bound")
    if not kf.is_in_image(u, v, rules):
        _hit(hits, "outside_image")
        return SKIPPED, -1, -1
    max_d, min_d = f32(f32(1.2) * mp.max_d), f32(f32(0.8) * mp.min_d)
    PO = [f32(p[i] - Ow[i]) for i in range(3)]
    dist3d = f32(MR.normd(PO, MR.Rules(norm=rules.norm)))
    if dist3d == min_d:
        _hit(hits, "on_depth_min")
    if dist3d == max_d:
        _hit(hits, "on_depth_max")
    if dist3d < min_d or dist3d > max_d:
        _hit(hits, "depth_low" if dist3d < min_d else "depth_high")
        return SKIPPED, -1, -1
    if MR.dotd(PO, mp.normal, MR.Rules(norm=rules.dot)) < 0.5 * f64(dist3d):
        _hit(hits, "angle")
        return SKIPPED, -1, -1
    level = predict_scale(mp.max_d, dist3d, kf.log_sf, kf.nlevels, _LOG_F())
    radius = f32(f32(th) * f32(kf.sf[level]))
    idxs = kf.features_in_area(u, v, radius, hits)
    if not idxs:
        _hit(hits, "no_candidate")
        return SKIPPED, -1, -1
    dmp = int.from_bytes(mp.desc.tobytes(), "little")
    best_dist, best_idx = 256, -1
    hi = level + 1 if rules.levels == "l+1" else level
    for idx in idxs:
        kp = kf.keys[idx]
        o = int(kp["octave"])
        if o == level + 1:
            _hit(hits, "octave_above")
        if o < level - 1 or o > hi:
            continue
        ex, ey = f32(u - f32(kp["x"])), f32(v - f32(kp["y"]))
        e2 = f32(f32(ex * ex) + f32(ey * ey))
        chi = f32(e2 * f32(kf.inv_sigma2[o]))
        if float(chi) > 5.99:
            _hit(hits, "chi2")
            continue
        if float(chi) > 5.0:
            _hit(hits, "chi2_near")
        dist = _dist(dmp, kf.dint[idx])
        if dist == best_dist:
            _hit(hits, "tie")
        if dist < best_dist or (rules.tie == "last" and dist == best_dist):
            best_dist, best_idx = dist, idx
    if best_dist in (TH_LOW, TH_LOW + 1):
        _hit(hits, "dist_%d" % best_dist)
    if not (best_dist < TH_LOW if rules.th_low == "lt" else best_dist <= TH_LOW):
        _hit(hits, "no_match")
        return NO_MATCH, best_idx, best_dist
    return MATCHED, best_idx, best_dist


def fuse(kf, points, th=3.0, rules=REFERENCE, hits=None, trace=None):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:827-979), sequential.  Returns nFused; `trace` (a list or None)
    receives per query (action, bestIdx, bestDist) as pgorb_fuse reports them."""
    nfused = 0
    for mp in points:
        a, bi, bd = match(kf, mp, th, rules, hits)
        if a != MATCHED:
            if trace is not None:
                trace.append((a, bi, bd))
            continue
        occ = kf.slots[bi]
        if occ is not None:
            if not occ.bad:
                if occ.observations() == mp.observations():
                    _hit(hits, "obs_tie")
                if len(occ.obs) == 1 + len(mp.obs) and set(occ.obs) & set(mp.obs):
                    _hit(hits, "overlap")
                keep = occ.observations() >= mp.observations() if rules.obs_cmp == "ge" else occ.observations() > mp.observations()
                if keep:
                    _hit(hits, "merged")
                    mp.replace(occ, rules)                                   # the query becomes bad
                    a = MERGED
                else:
                    _hit(hits, "replaced")
                    occ.replace(mp, rules)                                   # the query takes the slot
                    a = REPLACED
            else:
                _hit(hits, "kf_point_bad")
                a = KF_POINT_BAD
        else:
            _hit(hits, "added")
            mp.add_observation(kf, bi)                                       # AddObservation + AddMapPoint
            kf.slots[bi] = mp
            a = ADDED
        if trace is not None:
            trace.append((a, bi, bd))
        nfused += 1
    return nfused


_log_f = None


def _LOG_F():
    global _log_f
    if _log_f is None:
        from matcher_reference import contract_log_f
        _log_f = contract_log_f()
    return _log_f


def search_in_neighbors(current, targets, th=3.0, rules=REFERENCE, hits=None):
    """The two Fuse rounds of LocalMapping::SearchInNeighbors (LocalMapping.cc:487-516) over the given targets, without the
    final per-point update (:521-532).  Returns the nFused of each call."""
    res = []
    vp = list(current.slots)                                                  # GetMapPointMatches()
    for kf in targets:
        res.append(fuse(kf, vp, th, rules, hits))
    cand, seen = [], set()
    for kf in targets:
        for mp in list(kf.slots):
            if mp is None or mp.bad or mp.id in seen:
                continue
            seen.add(mp.id)
            cand.append(mp)
    res.append(fuse(current, cand, th, rules, hits))
    return res


# ---------------------------------------------------------------- the two-pass form (the kernels' specification)
def fuse_two_pass(kf, points, th=3.0):
    """pgorb_fuse's decomposition on plain objects: every query matched against the state on entry, then each slot's chain
    walked in query order with the observation sets as unions of key-frame ids.  Changes nothing; returns (nFused,
    [(action, bestIdx, bestDist)], slots afterwards)."""
    first = [match(kf, mp, th) for mp in points]                             # pass 1: no query depends on another
    slots = list(kf.slots)
    union = {}
    acts, nf = [], 0
    for q, (a, bi, bd) in enumerate(first):                                  # pass 2: per slot, in query order
        if a != MATCHED:
            acts.append((a, bi, bd))
            continue
        nf += 1
        mine = {k.id for k in points[q].obs}
        occ0 = kf.slots[bi]
        if occ0 is not None and occ0.bad:
            acts.append((KF_POINT_BAD, bi, bd))
            continue
        if bi not in union and occ0 is None:
            union[bi] = mine | {kf.id}
            slots[bi] = points[q]
            acts.append((ADDED, bi, bd))
            continue
        if bi not in union:
            union[bi] = {k.id for k in occ0.obs}
        u = union[bi]
        if len(u) > len(mine):
            acts.append((MERGED, bi, bd))
        else:
            acts.append((REPLACED, bi, bd))
            slots[bi] = points[q]
        u |= mine
    return nf, acts, slots
