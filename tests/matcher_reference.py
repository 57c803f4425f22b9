"""A plain, sequential restatement of the Frame grid and the guided matchers, written from the upstream text
(thirdparty/orb-slam2/src/Frame.cc, ORBmatcher.cc, MapPoint.cc) and nothing else: it does not use oracle/ and was not
derived from the oracle's C or from the HIP kernels, so a misreading of the upstream code shared by those two sides shows
up as a disagreement here.

Conventions:
- Arguments follow the ABI wrappers of pilotguru_amd/orb.py: keypoints are KEYPOINT_DTYPE arrays, descriptors [n, 32]
  uint8, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), scale factors have nlevels + 1 entries, feature vectors are the
  (nodes, starts, features) triples of ORBVocabulary.transform(), and a matcher returns (nmatches, assignment array).
- Every loop runs in the reference's own order and every tie is left to the reference's strict `<` comparisons.
- Every value the reference computes in `float` is an np.float32 scalar, evaluated in the same order; `round` is C's
  (half away from zero), `floor` / `ceil` are followed by an int conversion, (float)INT_MAX is 2147483648.0f.
- `rules` (a Rules) switches single rules to a wrong reading; the defaults are the reference's behaviour.  The mutation
  test of tests/test_matcher_edges.py shows that the constructed cases tell every switch from the reference.
- `hits` (a collections.Counter, or None) counts the edges a call reached, so a test can assert that its case family
  really exercised the rule it targets.
"""
import bisect
import math
from dataclasses import dataclass

import numpy as np

f32 = np.float32
GRID_COLS, GRID_ROWS = 64, 48                    # include/Frame.h:37-38
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30      # ORBmatcher.cc:38-40
INT_MAX = 2 ** 31 - 1
ROT_FACTOR = f32(1.0) / f32(HISTO_LENGTH)        # const float factor = 1.0f/HISTO_LENGTH (:170, :414, :1339, :1488)


@dataclass(frozen=True)
class Rules:
    tie_order: str = "cell"          # GetFeaturesInArea's (column, row, insertion) order | "index": ascending keypoint index
    rounding: str = "half_away"      # C round() in PosInGrid and the rotation bin | "half_even"
    window: str = "strict"           # fabs(distx) < r (Frame.cc:377) | "inclusive": <=
    threshold: str = "le"            # bestDist <= TH_LOW / TH_HIGH / ORBdist | "lt"
    ratio: str = "float"             # ratio tests in float | "double"
    three_maxima: str = "float"      # max2 < 0.1f*(float)max1 | "double": the product 0.1f * max1 in double | "le": <=
    sfi_replace: str = "lower"       # SFI takes an F2 keypoint on a strictly lower distance (:445) | "equal": also on ties


REFERENCE = Rules()
MUTANTS = {
    "tie_order=index": Rules(tie_order="index"),
    "rounding=half_even": Rules(rounding="half_even"),
    "window=inclusive": Rules(window="inclusive"),
    "threshold=lt": Rules(threshold="lt"),
    "ratio=double": Rules(ratio="double"),
    "three_maxima=double": Rules(three_maxima="double"),
    "three_maxima=le": Rules(three_maxima="le"),
    "sfi_replace=equal": Rules(sfi_replace="equal"),
}


def _hit(hits, key, n=1):
    if hits is not None:
        hits[key] += n


def c_round(v, rules=REFERENCE):
    """C round(): half away from zero (exact for float inputs: |v| + 0.5 is exact in double)."""
    v = float(v)
    if rules.rounding == "half_even":
        return int(round(v))
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def _is_half(v):
    v = float(v)
    return v - math.floor(v) == 0.5


def descriptor_ints(desc):
    """Descriptors as Python integers (Hamming distance = popcount of the xor, ORBmatcher::DescriptorDistance)."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") for row in d]


def _dist(a, b):
    return (a ^ b).bit_count()


def _within(th, d, rules):
    return d < th if rules.threshold == "lt" else d <= th


# ---------------------------------------------------------------- Frame grid (Frame.cc)
class Grid:
    """Frame::AssignFeaturesToGrid (Frame.cc:234-249) with PosInGrid (:386-396), and GetFeaturesInArea (:331-384)."""

    def __init__(self, keys, bounds, rules=REFERENCE, hits=None):
        self.keys = np.ascontiguousarray(keys)
        self.rules = rules
        self.min_x, self.max_x, self.min_y, self.max_y = (f32(b) for b in bounds)
        # mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS)/(mnMaxX-mnMinX) (Frame.cc:105-106, :159-160)
        self.inv_w = f32(GRID_COLS) / f32(self.max_x - self.min_x)
        self.inv_h = f32(GRID_ROWS) / f32(self.max_y - self.min_y)
        self.cells = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(len(self.keys)):
            pos = self.pos_in_grid(self.keys["x"][i], self.keys["y"][i], hits)
            if pos is not None:
                self.cells[pos[0]][pos[1]].append(i)

    def pos_in_grid(self, x, y, hits=None):
        gx = f32(f32(f32(x) - self.min_x) * self.inv_w)
        gy = f32(f32(f32(y) - self.min_y) * self.inv_h)
        if _is_half(gx) or _is_half(gy):
            _hit(hits, "grid_half_cell")
        px, py = c_round(gx, self.rules), c_round(gy, self.rules)
        if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
            _hit(hits, "grid_rejected")
            return None
        return px, py

    def csr(self):
        """The ABI's CSR form: start[3073] over cells col*48 + row, indices in insertion order."""
        start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32)
        idx = []
        for c in range(GRID_COLS):
            for r in range(GRID_ROWS):
                idx.extend(self.cells[c][r])
                start[c * GRID_ROWS + r + 1] = len(idx)
        return start, np.array(idx, np.int32)

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1, hits=None):
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        lo_x = math.floor(f32(f32(x - self.min_x) - r) * self.inv_w)
        min_cx = max(0, int(lo_x))
        if min_cx >= GRID_COLS:
            _hit(hits, "area_empty_right")
            return out
        max_cx = min(GRID_COLS - 1, int(math.ceil(f32(f32(x - self.min_x) + r) * self.inv_w)))
        if max_cx < 0:
            _hit(hits, "area_empty_left")
            return out
        min_cy = max(0, int(math.floor(f32(f32(y - self.min_y) - r) * self.inv_h)))
        if min_cy >= GRID_ROWS:
            _hit(hits, "area_empty_bottom")
            return out
        max_cy = min(GRID_ROWS - 1, int(math.ceil(f32(f32(y - self.min_y) + r) * self.inv_h)))
        if max_cy < 0:
            _hit(hits, "area_empty_top")
            return out
        check_levels = min_level > 0 or max_level >= 0
        if min_level < 0 and max_level >= 0:
            _hit(hits, "area_level_floor_open")
        kx, ky, ko = self.keys["x"], self.keys["y"], self.keys["octave"]
        for cx in range(min_cx, max_cx + 1):
            for cy in range(min_cy, max_cy + 1):
                for i in self.cells[cx][cy]:
                    if check_levels:
                        if ko[i] < min_level:
                            continue
                        if max_level >= 0 and ko[i] > max_level:
                            continue
                    dx, dy = abs(f32(kx[i] - x)), abs(f32(ky[i] - y))
                    if dx == r or dy == r:
                        _hit(hits, "area_on_radius")
                    if self.rules.window == "inclusive":
                        inside = dx <= r and dy <= r
                    else:
                        inside = dx < r and dy < r
                    if inside:
                        out.append(i)
        if len(out) > 64:
            _hit(hits, "area_over_64")                  # more candidates than a query's fixed list slots in the kernel
        if len(out) > 64 + 256:
            _hit(hits, "area_over_320")                 # ... and than its share of the pooled list entries
        if self.rules.tie_order == "index":
            out.sort()
        elif any(out[k] > out[k + 1] for k in range(len(out) - 1)):
            _hit(hits, "area_order_not_index")
        return out


# ---------------------------------------------------------------- ORBmatcher helpers
def radius_by_viewing_cos(view_cos):
    """ORBmatcher::RadiusByViewingCos (ORBmatcher.cc:133-139): float against the double 0.998."""
    return f32(2.5) if float(f32(view_cos)) > 0.998 else f32(4.0)


def rotation_bin(angle_a, angle_b, rules=REFERENCE, hits=None):
    """rot = a - b (float), += 360 when negative, bin = round(rot*factor), 30 -> 0 (e.g. ORBmatcher.cc:467-472)."""
    rot = f32(f32(angle_a) - f32(angle_b))
    if rot < 0.0:
        _hit(hits, "rot_negative")
        rot = f32(rot + f32(360.0))
    v = f32(rot * ROT_FACTOR)
    if _is_half(v):
        _hit(hits, "rot_half_bin")
    b = c_round(v, rules)
    if b == HISTO_LENGTH:
        b = 0
    return b


def compute_three_maxima(sizes, rules=REFERENCE, hits=None):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1605-1646) on the bin sizes; returns (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
        elif s > 0 and s in (max1, max2, max3):
            _hit(hits, "hist_count_tie")

    def below(m):
        if rules.three_maxima == "double":
            return m < float(f32(0.1)) * max1
        lim = f32(f32(0.1) * f32(max1))
        if f32(m) == lim:
            _hit(hits, "hist_tenth_equal")
        return f32(m) <= lim if rules.three_maxima == "le" else f32(m) < lim

    if below(max2):
        ind2 = ind3 = -1
    elif below(max3):
        ind3 = -1
    return ind1, ind2, ind3


def _drop_outside_three_maxima(hist, rules, hits):
    """The bins ComputeThreeMaxima does not keep, in bin order."""
    keep = compute_three_maxima([len(h) for h in hist], rules, hits)
    _hit(hits, "hist_kept_bins", sum(k >= 0 for k in keep))
    return [i for i in range(HISTO_LENGTH) if i not in keep]


def _ratio_gt(best, nnratio, best2, rules):
    """bestDist > mfNNratio*bestDist2 (ORBmatcher.cc:122): int against a float product."""
    if rules.ratio == "double":
        return best > float(f32(nnratio)) * best2
    return f32(best) > f32(f32(nnratio) * f32(best2))


def _ratio_lt(best, nnratio, best2, rules):
    """static_cast<float>(bestDist1) < mfNNratio*static_cast<float>(bestDist2) (:230-232, :463)."""
    if rules.ratio == "double":
        return best < float(f32(nnratio)) * best2
    return f32(best) < f32(f32(nnratio) * f32(best2))


def _ratio_edge(best, nnratio, best2, hits):
    if f32(best) == f32(f32(nnratio) * f32(best2)) or best == float(f32(nnratio)) * best2 or \
            (f32(best) > f32(f32(nnratio) * f32(best2))) != (best > float(f32(nnratio)) * best2):
        _hit(hits, "ratio_boundary")


def predict_scale(max_distance, current_dist, log_scale_factor, nlevels, log_f, hits=None):
    """MapPoint::PredictScale (MapPoint.cc:516-531); `log_f` is the project's log contract (pgorb_log_f)."""
    ratio = f32(f32(max_distance) / f32(current_dist)) if f32(current_dist) != 0 else f32(np.inf)
    q = f32(f32(log_f(ratio)) / f32(log_scale_factor))
    c = math.ceil(q) if math.isfinite(q) else None
    n = -2 ** 31 if c is None else int(c)          # (int) of inf / nan: INT_MIN on x86-64
    if n < 0:
        _hit(hits, "predict_scale_clamped_low")
        n = 0
    elif n >= nlevels:
        n = nlevels - 1
    return n


# ---------------------------------------------------------------- the matchers
def search_by_projection_points(keys, desc, bounds, scale_factors, kp_has_point, valid, proj_x, proj_y, level, view_cos,
                                pdesc, pobs, th, nnratio, rules=REFERENCE, hits=None):
    """SearchByProjection(Frame &F, const vector<MapPoint*>&, th) (ORBmatcher.cc:46-131), monocular (mvuRight < 0).
    kp_has_point[i]: keypoint i holds a map point with Observations() > 0 before the call.  Returns (nmatches, assigned)
    with assigned[i] = the query written last to F.mvpMapPoints[i], or -1."""
    grid = Grid(keys, bounds, rules, hits)
    n = len(keys)
    dk, dq = descriptor_ints(desc), descriptor_ints(pdesc)
    sf = np.asarray(scale_factors, np.float32)
    blocked = [bool(kp_has_point[i]) if kp_has_point is not None else False for i in range(n)]
    assigned = [-1] * n
    th = f32(th)
    use_factor = th != f32(1.0)
    nmatches = 0
    for q in range(len(valid)):
        if not valid[q]:
            continue
        lvl = int(level[q])
        r = radius_by_viewing_cos(view_cos[q])
        if use_factor:
            r = f32(r * th)
        cand = grid.features_in_area(proj_x[q], proj_y[q], f32(r * sf[lvl]), lvl - 1, lvl, hits)
        if not cand:
            continue
        best, best_level, best2, best_level2, best_idx = 256, -1, 256, -1, -1
        for i in cand:
            if blocked[i]:
                _hit(hits, "candidate_blocked")
                continue
            d = _dist(dq[q], dk[i])
            if d < best:
                best2, best = best, d
                best_level2, best_level = best_level, int(keys["octave"][i])
                best_idx = i
            else:
                if d == best:
                    _hit(hits, "tie_best")
                if d < best2:
                    best_level2, best2 = int(keys["octave"][i]), d
        if best in (TH_HIGH, TH_HIGH + 1):
            _hit(hits, "threshold_edge")
        if best2 == 256 and best < 256:
            _hit(hits, "single_candidate")
        if _within(TH_HIGH, best, rules):
            if best == best2:
                _hit(hits, "ratio_gate_same_level" if best_level == best_level2 else "ratio_gate_other_level")
            if best_level == best_level2:
                _ratio_edge(best, nnratio, best2, hits)
                if _ratio_gt(best, nnratio, best2, rules):
                    continue
            if assigned[best_idx] >= 0:
                _hit(hits, "overwrite_without_observations")
            assigned[best_idx] = q
            blocked[best_idx] = bool(pobs[q])
            nmatches += 1
    return nmatches, np.array(assigned, np.int32)


def search_by_projection_frame(keys, desc, bounds, scale_factors, kp_has_point, valid, u, v, last_octave, last_angle,
                               pdesc, pobs, th, check_orientation=True, rules=REFERENCE, hits=None):
    """The matching loop of SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) (ORBmatcher.cc:1355-1474)
    for given projections; `valid` already holds the pose and image-bounds tests (:1364-1385)."""
    grid = Grid(keys, bounds, rules, hits)
    n = len(keys)
    dk, dq = descriptor_ints(desc), descriptor_ints(pdesc)
    sf = np.asarray(scale_factors, np.float32)
    blocked = [bool(kp_has_point[i]) if kp_has_point is not None else False for i in range(n)]
    assigned = [-1] * n
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for q in range(len(valid)):
        if not valid[q]:
            continue
        octave = int(last_octave[q])
        radius = f32(f32(th) * sf[octave])
        cand = grid.features_in_area(u[q], v[q], radius, octave - 1, octave + 1, hits)
        if not cand:
            continue
        best, best_idx = 256, -1
        for i in cand:
            if blocked[i]:
                _hit(hits, "candidate_blocked")
                continue
            d = _dist(dq[q], dk[i])
            if d < best:
                best, best_idx = d, i
            elif d == best:
                _hit(hits, "tie_best")
        if best in (TH_HIGH, TH_HIGH + 1):
            _hit(hits, "threshold_edge")
        if _within(TH_HIGH, best, rules):
            assigned[best_idx] = q
            blocked[best_idx] = bool(pobs[q])
            nmatches += 1
            if check_orientation:
                hist[rotation_bin(last_angle[q], keys["angle"][best_idx], rules, hits)].append(best_idx)
    if check_orientation:
        for b in _drop_outside_three_maxima(hist, rules, hits):
            for i in hist[b]:
                assigned[i] = -1
                nmatches -= 1
    return nmatches, np.array(assigned, np.int32)


def search_by_projection_keyframe(keys, desc, bounds, scale_factors, kp_has_point, valid, found, u, v, dist3d,
                                  min_distance, max_distance, log_scale_factor, kf_angle, pdesc, th, orb_dist,
                                  check_orientation=True, log_f=None, rules=REFERENCE, hits=None):
    """The matching loop of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1476-1603)
    from the projections on: image bounds (:1512-1515), depth range (:1519-1526), PredictScale, window, best match only.
    min_distance / max_distance are the points' mfMinDistance / mfMaxDistance: the depth range is 0.8f*min .. 1.2f*max
    (GetMin/MaxDistanceInvariance), PredictScale divides the plain max.
    Any point in CurrentFrame.mvpMapPoints blocks a keypoint (:1542-1543).  nlevels = len(scale_factors) - 1."""
    if log_f is None:
        log_f = contract_log_f()
    grid = Grid(keys, bounds, rules, hits)
    n = len(keys)
    dk, dq = descriptor_ints(desc), descriptor_ints(pdesc)
    sf = np.asarray(scale_factors, np.float32)
    nlevels = len(sf) - 1
    held = [bool(kp_has_point[i]) if kp_has_point is not None else False for i in range(n)]
    assigned = [-1] * n
    hist = [[] for _ in range(HISTO_LENGTH)]
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    nmatches = 0
    for q in range(len(valid)):
        if not valid[q] or found[q]:
            continue
        uq, vq = f32(u[q]), f32(v[q])
        if uq < min_x or uq > max_x or vq < min_y or vq > max_y:
            continue
        if uq == min_x or uq == max_x or vq == min_y or vq == max_y:
            _hit(hits, "projection_on_bounds")
        d3, dmin, dmax = f32(dist3d[q]), f32(min_distance[q]), f32(max_distance[q])
        if d3 < f32(f32(0.8) * dmin) or d3 > f32(f32(1.2) * dmax):     # GetMin/MaxDistanceInvariance (MapPoint.cc:390-400)
            continue
        if d3 > dmax:
            _hit(hits, "predict_ratio_below_one")                       # depth in (mfMaxDistance, 1.2f*mfMaxDistance]
        lvl = predict_scale(dmax, d3, log_scale_factor, nlevels, log_f, hits)   # the plain mfMaxDistance (MapPoint.cc:521)
        if lvl == 0:
            _hit(hits, "predicted_level_first")
        if lvl == nlevels - 1:
            _hit(hits, "predicted_level_last")
        radius = f32(f32(th) * sf[lvl])
        cand = grid.features_in_area(uq, vq, radius, lvl - 1, lvl + 1, hits)
        if not cand:
            continue
        best, best_idx = 256, -1
        for i in cand:
            if held[i]:
                _hit(hits, "candidate_blocked")
                continue
            d = _dist(dq[q], dk[i])
            if d < best:
                best, best_idx = d, i
            elif d == best:
                _hit(hits, "tie_best")
        if best in (orb_dist, orb_dist + 1):
            _hit(hits, "threshold_edge")
        if _within(orb_dist, best, rules):
            assigned[best_idx] = q
            held[best_idx] = True
            nmatches += 1
            if check_orientation:
                hist[rotation_bin(kf_angle[q], keys["angle"][best_idx], rules, hits)].append(best_idx)
    if check_orientation:
        for b in _drop_outside_three_maxima(hist, rules, hits):
            for i in hist[b]:
                assigned[i] = -1
                nmatches -= 1
    return nmatches, np.array(assigned, np.int32)


def search_by_bow(kf_desc, kf_angle, kf_valid, kf_fv, f_desc, f_angle, f_fv, nnratio, check_orientation=True,
                  rules=REFERENCE, hits=None):
    """SearchByBoW(KeyFrame* pKF, Frame &F, vpMapPointMatches) (ORBmatcher.cc:161-290).  Returns (nmatches, matches)
    with matches[j] = the key-frame keypoint whose map point went to vpMapPointMatches[j], or -1."""
    dk, df = descriptor_ints(kf_desc), descriptor_ints(f_desc)
    k_nodes, k_start, k_feat = [np.asarray(a) for a in kf_fv]
    f_nodes, f_start, f_feat = [np.asarray(a) for a in f_fv]
    k_nodes, f_nodes = [int(x) for x in k_nodes], [int(x) for x in f_nodes]
    matches = [-1] * len(df)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    a = b = 0
    while a < len(k_nodes) and b < len(f_nodes):
        if k_nodes[a] == f_nodes[b]:
            for kf_i in k_feat[k_start[a]:k_start[a + 1]]:
                kf_i = int(kf_i)
                if not kf_valid[kf_i]:
                    continue
                best1, best_idx, best2 = 256, -1, 256
                for f_i in f_feat[f_start[b]:f_start[b + 1]]:
                    f_i = int(f_i)
                    if matches[f_i] >= 0:
                        _hit(hits, "candidate_blocked")
                        continue
                    d = _dist(dk[kf_i], df[f_i])
                    if d < best1:
                        best2, best1, best_idx = best1, d, f_i
                    else:
                        if d == best1:
                            _hit(hits, "tie_best")
                        if d < best2:
                            best2 = d
                if best1 in (TH_LOW, TH_LOW + 1):
                    _hit(hits, "threshold_edge")
                if _within(TH_LOW, best1, rules):
                    _ratio_edge(best1, nnratio, best2, hits)
                    if _ratio_lt(best1, nnratio, best2, rules):
                        matches[best_idx] = kf_i
                        if check_orientation:
                            hist[rotation_bin(kf_angle[kf_i], f_angle[best_idx], rules, hits)].append(best_idx)
                        nmatches += 1
            a += 1
            b += 1
        elif k_nodes[a] < f_nodes[b]:
            a = bisect.bisect_left(k_nodes, f_nodes[b])          # lower_bound (:263)
        else:
            b = bisect.bisect_left(f_nodes, k_nodes[a])          # (:267)
    if check_orientation:
        for bn in _drop_outside_three_maxima(hist, rules, hits):
            for j in hist[bn]:
                matches[j] = -1
                nmatches -= 1
    return nmatches, np.array(matches, np.int32)


def search_for_initialization(keys1, desc1, keys2, desc2, bounds, prev_matched, window_size=100, nnratio=0.9,
                              check_orientation=True, rules=REFERENCE, hits=None):
    """ORBmatcher::SearchForInitialization (ORBmatcher.cc:407-522).  Returns (nmatches, vnMatches12, vbPrevMatched) with
    vbPrevMatched a float32 [n1, 2] copy updated as the reference updates it."""
    grid = Grid(keys2, bounds, rules, hits)
    n1, n2 = len(keys1), len(keys2)
    d1, d2 = descriptor_ints(desc1), descriptor_ints(desc2)
    prev = np.array(prev_matched, np.float32).reshape(n1, 2).copy()
    m12 = [-1] * n1
    matched_dist = [INT_MAX] * n2
    m21 = [-1] * n2
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i1 in range(n1):
        level1 = int(keys1["octave"][i1])
        if level1 > 0:
            _hit(hits, "sfi_skipped_level")
            continue
        cand = grid.features_in_area(prev[i1, 0], prev[i1, 1], f32(window_size), level1, level1, hits)
        if not cand:
            continue
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for i2 in cand:
            d = _dist(d1[i1], d2[i2])
            if matched_dist[i2] == d:
                _hit(hits, "sfi_equal_to_taken")
            if matched_dist[i2] < d if rules.sfi_replace == "equal" else matched_dist[i2] <= d:
                continue
            if d < best:
                best2, best, best_idx = best, d, i2
            else:
                if d == best:
                    _hit(hits, "tie_best")
                if d < best2:
                    best2 = d
        if best in (TH_LOW, TH_LOW + 1):
            _hit(hits, "threshold_edge")
        if best2 == INT_MAX and best < INT_MAX:
            _hit(hits, "single_candidate")
        if _within(TH_LOW, best, rules):
            _ratio_edge(best, nnratio, best2, hits)
            if _ratio_lt(best, nnratio, best2, rules):
                if m21[best_idx] >= 0:
                    _hit(hits, "sfi_steal")
                    m12[m21[best_idx]] = -1
                    nmatches -= 1
                m12[i1] = best_idx
                m21[best_idx] = i1
                matched_dist[best_idx] = best
                nmatches += 1
                if check_orientation:
                    hist[rotation_bin(keys1["angle"][i1], keys2["angle"][best_idx], rules, hits)].append(i1)
    if check_orientation:
        for b in _drop_outside_three_maxima(hist, rules, hits):
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nmatches -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1, 0] = keys2["x"][m12[i1]]
            prev[i1, 1] = keys2["y"][m12[i1]]
    return nmatches, np.array(m12, np.int32), prev


def contract_log_f():
    """The project's published log contract (pgorb_log_f, equal to orc_log_f per test_log_contract_and_predict_scale)."""
    import ctypes as C
    from pilotguru_amd import _lib
    L = _lib.lib()
    return lambda x: float(L.pgorb_log_f(C.c_float(float(x))))
