"""A plain, sequential restatement of ORBmatcher::SearchForTriangulation (thirdparty/orb-slam2/src/ORBmatcher.cc:659-825) with
CheckDistEpipolarLine (:142-159), written from that upstream text and nothing else: it does not use oracle/ and was not derived
from the HIP kernel (pilotguru_amd/csrc/node_match.hip), so a misreading shared by neither side shows up as a disagreement.

Conventions (those of tests/matcher_reference.py):
- Keypoints are KEYPOINT_DTYPE arrays (the undistorted mvKeysUn), descriptors [n, 32] uint8, feature vectors the
  (nodes, starts, features) triples of ORBVocabulary.transform(), F12 a 3x3 float32 array (F12.at<float>(r, c) = F12[r, c]),
  epipole = (ex, ey), scale factors / level sigma^2 the extractor's tables (nlevels + 1 entries).  Monocular: bOnlyStereo =
  false and mvuRight < 0, so the epipole test always runs (:745-751).
- Loops run in the reference's order; every value the reference computes in `float` is an np.float32 scalar evaluated in the
  same order; `3.84*mvLevelSigma2[o]` and the comparison with it are double (:158).
- has_point1 / has_point2: GetMapPoint(i) != NULL (:701-705, :724-728).
- `rules` (a Rules) switches single rules to a wrong reading; `hits` (a collections.Counter or None) counts the edges reached.
"""
import bisect
import math
import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from matcher_reference import HISTO_LENGTH, ROT_FACTOR, TH_LOW, _dist, _hit, c_round, compute_three_maxima, descriptor_ints  # noqa: E402

f32 = np.float32


@dataclass(frozen=True)
class Rules:
    matched2: str = "never_set"      # vbMatched2 is read (:727) but never set | "set": a matched KF2 keypoint blocks later KF1 keypoints
    tie: str = "last"                # `dist > bestDist` skips (:740), so an equal later candidate that passes replaces | "first"
    best_update: str = "geometry"    # bestDist moves only when both geometric tests pass (:753-757) | "before": before the tests
    line_compare: str = "double"     # dsqr < 3.84*mvLevelSigma2[o] in double (:158) | "float": 3.84f, float comparison
    epipole: str = "lt"              # reject on distex^2 + distey^2 < 100*scale (:749) | "le"
    threshold: str = "le"            # `dist > TH_LOW` skips, so 50 is kept (:740) | "lt"


REFERENCE = Rules()
MUTANTS = {
    "matched2=set": Rules(matched2="set"),
    "tie=first": Rules(tie="first"),
    "best_update=before": Rules(best_update="before"),
    "line_compare=float": Rules(line_compare="float"),
    "epipole=le": Rules(epipole="le"),
    "threshold=lt": Rules(threshold="lt"),
}


def level_sigma2(scale_factors):
    """mvLevelSigma2[i] = mvScaleFactor[i]*mvScaleFactor[i] (float, ORBextractor.cc)."""
    return np.array([f32(f32(s) * f32(s)) for s in scale_factors], np.float32)


def epipole_rejects(ex, ey, x2, y2, scale, rules=REFERENCE, hits=None):
    """distex*distex + distey*distey < 100*mvScaleFactors[octave] (:745-751), float."""
    with np.errstate(all="ignore"):
        dx, dy = f32(f32(ex) - f32(x2)), f32(f32(ey) - f32(y2))
        d2 = f32(f32(dx * dx) + f32(dy * dy))
        lim = f32(f32(100) * f32(scale))
    if not (math.isfinite(float(ex)) and math.isfinite(float(ey))):
        _hit(hits, "epipole_nonfinite")
    if d2 == lim:
        _hit(hits, "epipole_equal")
    rej = d2 <= lim if rules.epipole == "le" else d2 < lim
    if rej:
        _hit(hits, "epipole_rejected")
    return bool(rej)


def check_dist_epipolar_line(x1, y1, x2, y2, F, sigma2, rules=REFERENCE, hits=None):
    """CheckDistEpipolarLine (:142-159): the line l = x1'F12 = [a b c], num, den in float; dsqr < 3.84*sigma2 in double."""
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    with np.errstate(all="ignore"):
        a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
        b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
        c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
        num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
        den = f32(f32(a * a) + f32(b * b))
        if den == 0:
            _hit(hits, "den_zero")
            if np.signbit(a) or np.signbit(b):
                _hit(hits, "den_zero_negative_coefficient")
            return False
        if 0 < abs(float(den)) < float(np.finfo(np.float32).tiny):
            _hit(hits, "den_subnormal")
        dsqr = f32(f32(num * num) / den)
        lim_d = 3.84 * float(f32(sigma2))
        lim_f = f32(f32(3.84) * f32(sigma2))
    in_double, in_float = float(dsqr) < lim_d, bool(dsqr < lim_f)
    if in_double != in_float:
        _hit(hits, "line_float_double_differ")
    ok = in_float if rules.line_compare == "float" else in_double
    if not ok:
        _hit(hits, "line_rejected")
    return ok


def _rotation_bin(angle1, angle2, hits):
    """rot = kp1.angle - kp2.angle, += 360 when negative, round(rot*factor), 30 -> 0 (:764-776)."""
    rot = f32(f32(angle1) - f32(angle2))
    if rot < 0.0:
        _hit(hits, "rot_negative")
        rot = f32(rot + f32(360.0))
    b = c_round(f32(rot * ROT_FACTOR))
    if b == HISTO_LENGTH:
        _hit(hits, "rot_bin_30")
        b = 0
    return b


def search_for_triangulation(keys1, desc1, has1, fv1, keys2, desc2, has2, fv2, F12, epipole, scale_factors, sigma2,
                             check_orientation=True, rules=REFERENCE, hits=None):
    """Returns (nmatches, matches12) with matches12[i] = vMatches12[i] (the KF2 keypoint of KF1 keypoint i, or -1)."""
    d1, d2 = descriptor_ints(desc1), descriptor_ints(desc2)
    n1, n2 = len(keys1), len(keys2)
    has1 = np.zeros(n1, np.uint8) if has1 is None else np.asarray(has1)
    has2 = np.zeros(n2, np.uint8) if has2 is None else np.asarray(has2)
    F = np.asarray(F12, np.float32).reshape(3, 3)
    ex, ey = f32(epipole[0]), f32(epipole[1])
    nodes1, start1, feat1 = [np.asarray(a) for a in fv1]
    nodes2, start2, feat2 = [np.asarray(a) for a in fv2]
    nodes1, nodes2 = [int(x) for x in nodes1], [int(x) for x in nodes2]
    matched2 = [False] * n2
    matches12 = [-1] * n1
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    common = 0
    a = b = 0
    while a < len(nodes1) and b < len(nodes2):
        if nodes1[a] == nodes2[b]:
            common += 1
            cands = [int(j) for j in feat2[start2[b]:start2[b + 1]]]
            if len(cands) > 256:
                _hit(hits, "node_over_256")
            for idx1 in feat1[start1[a]:start1[a + 1]]:
                idx1 = int(idx1)
                if has1[idx1]:
                    _hit(hits, "kf1_has_point")
                    continue
                kp1 = keys1[idx1]
                best_dist, best_idx = TH_LOW, -1
                for idx2 in cands:
                    if matched2[idx2] or has2[idx2]:
                        _hit(hits, "kf2_matched" if matched2[idx2] else "kf2_has_point")
                        continue
                    dist = _dist(d1[idx1], d2[idx2])
                    over = dist >= TH_LOW if rules.threshold == "lt" else dist > TH_LOW
                    if dist in (TH_LOW, TH_LOW + 1):
                        _hit(hits, "dist_%d" % dist)
                    if over or dist > best_dist:
                        continue
                    if best_idx >= 0 and dist == best_dist:
                        _hit(hits, "tie_candidate")
                        if rules.tie == "first":
                            continue
                    if rules.best_update == "before":
                        best_dist = dist
                    kp2 = keys2[idx2]
                    o = int(kp2["octave"])
                    if epipole_rejects(ex, ey, kp2["x"], kp2["y"], scale_factors[o], rules, hits):
                        continue
                    if check_dist_epipolar_line(kp1["x"], kp1["y"], kp2["x"], kp2["y"], F, sigma2[o], rules, hits):
                        if best_idx >= 0 and dist == best_dist:
                            _hit(hits, "tie_later_wins")
                        best_idx, best_dist = idx2, dist
                    elif best_idx < 0 and dist < best_dist:
                        _hit(hits, "closer_candidate_failed")
                if best_idx >= 0:
                    if best_dist == TH_LOW:
                        _hit(hits, "kept_at_threshold")
                    matches12[idx1] = best_idx
                    nmatches += 1
                    if rules.matched2 == "set":
                        matched2[best_idx] = True
                    if check_orientation:
                        hist[_rotation_bin(kp1["angle"], keys2[best_idx]["angle"], hits)].append(idx1)
            a += 1
            b += 1
        elif nodes1[a] < nodes2[b]:
            a = bisect.bisect_left(nodes1, nodes2[b])          # lower_bound (:785)
        else:
            b = bisect.bisect_left(nodes2, nodes1[a])          # (:789)
    if not common:
        _hit(hits, "no_common_node")
    if check_orientation:                                      # :793-812
        keep = compute_three_maxima([len(h) for h in hist], hits=hits)
        for bn in range(HISTO_LENGTH):
            if bn in keep:
                continue
            for i in hist[bn]:
                _hit(hits, "hist_dropped")
                matches12[i] = -1
                nmatches -= 1
    taken = [j for j in matches12 if j >= 0]
    if len(set(taken)) < len(taken):
        _hit(hits, "kf2_shared")
    return nmatches, np.array(matches12, np.int32)


def matched_pairs(matches12):
    """vMatchedPairs (:814-822): (i, matches12[i]) for ascending i with a match."""
    return [(i, int(j)) for i, j in enumerate(matches12) if j >= 0]
