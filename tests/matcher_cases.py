"""Constructed edge cases of the Frame grid and the guided matchers (pilotguru_amd/csrc/frame.hip, init_match.hip, window_match.hip,
node_match.hip) and the runners that put them through the plain reference (tests/matcher_reference.py), the oracle, the single-call ABI and the batched device forms.
A helper module (no tests): tests/test_matcher_edges.py and the matcher_edges fuzzer of tests/fuzzers.py use it.

Frames are built straight from arrays, with descriptors at exact Hamming distances from their queries.  Families:
  a ties (cell order is not keypoint order)        b thresholds and ratio products     c window / grid geometry
  d pyramid levels and PredictScale                 e rotation histogram               f conflicts between queries
  g the kernel's list capacities (64 fixed slots, 256 pooled entries per query)"""
import collections
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_reference as R  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE  # noqa: E402
W, H = 640, 480
BOUNDS = (0.0, float(W), 0.0, float(H))
NLEVELS, SCALE = 8, 1.2
f32 = np.float32


def _scale_factors():
    """mvScaleFactors of an 8-level 1.2 pyramid as the extractor tables hold them (float products, nlevels + 1 entries)."""
    sf = [f32(1.0)]
    for _ in range(NLEVELS):
        sf.append(f32(sf[-1] * f32(SCALE)))
    return np.array(sf, np.float32)


SF = _scale_factors()


# ---------------------------------------------------------------- building frames from arrays
def keys(xs, ys, octave=0, angle=0.0):
    n = len(xs)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    k["octave"] = np.broadcast_to(np.asarray(octave, np.int32), n)
    k["angle"] = np.broadcast_to(np.asarray(angle, np.float32), n)
    k["size"], k["response"] = 31.0, 1.0
    return k


def at_distance(q, d, rng):
    """A descriptor exactly `d` bits away from q."""
    bits = np.unpackbits(q)
    flip = rng.choice(256, d, replace=False)
    bits[flip] ^= 1
    return np.packbits(bits)


def descs(q, dists, rng):
    return np.array([at_distance(q, int(d), rng) for d in dists], np.uint8).reshape(-1, 32)


def rand_desc(rng, n=1):
    return rng.randint(0, 256, (n, 32)).astype(np.uint8)


def _case(family, name, kind, **a):
    return dict(family=family, name=name, kind=kind, a=a)


def points_case(family, name, k, d, queries, th=1.0, ratio=0.8, has=None, bounds=BOUNDS):
    """queries: list of (x, y, level, view_cos, descriptor, has_obs)."""
    nq = len(queries)
    return _case(family, name, "points", keys=k, desc=d, bounds=bounds, has=has if has is not None else np.zeros(len(k), np.uint8),
                 valid=np.ones(nq, np.uint8), px=np.array([q[0] for q in queries], np.float32),
                 py=np.array([q[1] for q in queries], np.float32), lvl=np.array([q[2] for q in queries], np.int32),
                 vc=np.array([q[3] for q in queries], np.float32), pd=np.array([q[4] for q in queries], np.uint8).reshape(-1, 32),
                 obs=np.array([q[5] for q in queries], np.uint8), th=float(th), ratio=float(ratio))


def frame_case(family, name, k, d, queries, th=10.0, ori=True, has=None, bounds=BOUNDS):
    """queries: list of (u, v, last_octave, last_angle, descriptor, has_obs)."""
    nq = len(queries)
    return _case(family, name, "frame", keys=k, desc=d, bounds=bounds, has=has if has is not None else np.zeros(len(k), np.uint8),
                 valid=np.ones(nq, np.uint8), u=np.array([q[0] for q in queries], np.float32),
                 v=np.array([q[1] for q in queries], np.float32), oct=np.array([q[2] for q in queries], np.int32),
                 ang=np.array([q[3] for q in queries], np.float32), pd=np.array([q[4] for q in queries], np.uint8).reshape(-1, 32),
                 obs=np.array([q[5] for q in queries], np.uint8), th=float(th), ori=bool(ori))


def keyframe_case(family, name, k, d, queries, th=10.0, orbdist=100, ori=True, has=None, bounds=BOUNDS):
    """queries: list of (u, v, dist3d, min_distance, max_distance, kf_angle, descriptor, found)."""
    nq = len(queries)
    col = lambda j, dt: np.array([q[j] for q in queries], dt)
    return _case(family, name, "keyframe", keys=k, desc=d, bounds=bounds, has=has if has is not None else np.zeros(len(k), np.uint8),
                 valid=np.ones(nq, np.uint8), found=col(7, np.uint8), u=col(0, np.float32), v=col(1, np.float32),
                 d3=col(2, np.float32), mind=col(3, np.float32), maxd=col(4, np.float32), ang=col(5, np.float32),
                 pd=np.array([q[6] for q in queries], np.uint8).reshape(-1, 32), th=float(th), orbdist=int(orbdist), ori=bool(ori))


def sfi_case(family, name, k1, d1, k2, d2, prev=None, win=100, ratio=0.9, ori=True, bounds=BOUNDS):
    if prev is None:
        prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    return _case(family, name, "sfi", k1=k1, d1=d1, k2=k2, d2=d2, bounds=bounds, prev=np.asarray(prev, np.float32).reshape(-1, 2),
                 win=int(win), ratio=float(ratio), ori=bool(ori))


def _fv(node_of):
    """(nodes, starts, features) of a FeatureVector from each feature's node id (ascending nodes, features in order)."""
    nodes = sorted(set(int(x) for x in node_of))
    start, feat = [0], []
    for nd in nodes:
        feat.extend(i for i, x in enumerate(node_of) if int(x) == nd)
        start.append(len(feat))
    return np.array(nodes, np.uint32), np.array(start, np.int32), np.array(feat, np.uint32)


def bow_case(family, name, kk, kd, kvalid, knode, fk, fd, fnode, ratio=0.7, ori=True):
    return _case(family, name, "bow", kk=kk, kd=kd, kv=np.asarray(kvalid, np.uint8), kfv=_fv(knode), knode=np.asarray(knode, np.int32),
                 fk=fk, fd=fd, ffv=_fv(fnode), fnode=np.asarray(fnode, np.int32), ratio=float(ratio), ori=bool(ori))


# ---------------------------------------------------------------- the families
def _lattice(k):
    """Isolated positions 40 px apart (no window below 20 px reaches a neighbour)."""
    return 20.0 + 40.0 * (k % 15), 20.0 + 40.0 * (k // 15)


def family_a(rng):
    """Ties: equal minima where cell order and index order disagree, the ratio gate at equal distances, duplicate points."""
    out = []
    q = rand_desc(rng)[0]
    # index 0 sits in the higher column: GetFeaturesInArea returns index 1 first, and the first minimum wins
    k = keys([107.0, 93.0, 300.0], [100.0, 100.0, 300.0])
    d = descs(q, [30, 30, 5], rng)
    out.append(frame_case("a", "tie_across_columns_frame", k, d, [(100.0, 100.0, 0, 0.0, q, 1)], th=15.0, ori=False))
    out.append(keyframe_case("a", "tie_across_columns_keyframe", k, d, [(100.0, 100.0, 5.0, 1.0, 5.0, 0.0, q, 0)], th=15.0, ori=False))
    # same column, different rows: row order decides (index 0 in the lower row)
    k = keys([200.0, 200.0], [214.0, 186.0])
    out.append(frame_case("a", "tie_across_rows_frame", k, descs(q, [44, 44], rng), [(200.0, 200.0, 0, 0.0, q, 1)], th=20.0, ori=False))
    # bestDist == bestDist2 at the same level (the ratio gate rejects) and at different levels (accepted, cell order picks)
    k = keys([107.0, 93.0], [100.0, 100.0], octave=[1, 1])
    d = descs(q, [20, 20], rng)
    out.append(points_case("a", "tie_same_level_rejected_points", k, d, [(100.0, 100.0, 1, 0.9, q, 1)], th=10.0, ratio=0.9))   # 20 > 0.9f*20
    out.append(points_case("a", "tie_same_level_ratio_1_points", k, d, [(100.0, 100.0, 1, 0.9, q, 1)], th=10.0, ratio=1.0))   # 20 > 20 false
    k = keys([107.0, 93.0], [100.0, 100.0], octave=[1, 0])
    out.append(points_case("a", "tie_other_level_points", k, descs(q, [20, 20], rng), [(100.0, 100.0, 1, 0.9, q, 1)], th=10.0, ratio=0.6))
    # duplicate coordinates: one cell, insertion order; a second query finds the first one taken
    k = keys([250.0, 250.0, 250.0], [250.0, 250.0, 250.0], octave=[0, 0, 1])
    d = descs(q, [12, 12, 12], rng)
    out.append(frame_case("a", "duplicate_points_frame", k, d, [(251.0, 249.0, 0, 0.0, q, 1), (249.0, 251.0, 0, 0.0, q, 1)], th=5.0, ori=False))
    out.append(points_case("a", "duplicate_points_points", k, d, [(251.0, 249.0, 1, 0.999, q, 0), (249.0, 251.0, 1, 0.999, q, 1)], th=2.0))
    # SFI: equal minima reject through the ratio test; a third keypoint farther away is then irrelevant
    k1 = keys([100.0], [100.0])
    k2 = keys([107.0, 93.0, 100.0], [100.0, 100.0, 100.0])
    out.append(sfi_case("a", "tie_sfi", k1, q[None], k2, descs(q, [25, 25, 40], rng), win=20, ratio=1.0))
    return out


def family_b(rng):
    """Thresholds: TH_HIGH / TH_LOW / ORBdist at equality, ratio boundaries where the float product decides, single candidates."""
    out = []
    q = rand_desc(rng, 8)
    k = keys([_lattice(i)[0] for i in range(4)], [_lattice(i)[1] for i in range(4)])
    d = np.concatenate([descs(q[0], [100], rng), descs(q[1], [101], rng), descs(q[2], [99], rng), descs(q[3], [100], rng)])
    qs = [(_lattice(i)[0] + 1.0, _lattice(i)[1], 0, 0.0, q[i], 1) for i in range(4)]
    out.append(frame_case("b", "th_high_frame", k, d, qs, th=5.0, ori=False))
    out.append(points_case("b", "th_high_points", k, d, [(x, y, 0, 0.5, dd, 1) for x, y, _, _, dd, _ in qs], th=1.0))
    kq = [(x, y, 4.0, 1.0, 4.0, 0.0, dd, 0) for x, y, _, _, dd, _ in qs]
    out.append(keyframe_case("b", "orbdist_100_keyframe", k, d, kq, th=5.0, orbdist=100, ori=False))
    d64 = np.concatenate([descs(q[i], [dd], rng) for i, dd in enumerate([64, 65, 63, 64])])
    out.append(keyframe_case("b", "orbdist_64_keyframe", k, d64, [(x, y, 4.0, 1.0, 4.0, 0.0, q[i], 0) for i, (x, y, *_r) in enumerate(kq)],
                             th=3.0, orbdist=64, ori=False))
    # TH_LOW in SFI and BoW, single candidates (bestDist2 = INT_MAX / 256)
    k2 = keys([_lattice(i)[0] for i in range(4)], [_lattice(i)[1] for i in range(4)])
    d2 = np.concatenate([descs(q[i], [dd], rng) for i, dd in enumerate([50, 51, 49, 50])])
    k1 = keys([_lattice(i)[0] + 2 for i in range(4)], [_lattice(i)[1] for i in range(4)])
    out.append(sfi_case("b", "th_low_sfi", k1, q[:4], k2, d2, win=10, ratio=0.9))
    out.append(bow_case("b", "th_low_bow", k1, q[:4], [1, 1, 1, 1], [3, 5, 7, 9], k2, d2, [3, 5, 7, 9], ratio=0.9))
    # ratio products: best / second at 40 / 50 (0.8), 30 / 50 (0.6), 45 / 50 (0.9), in each form that has a ratio test
    for ratio, best in ((0.8, 40), (0.6, 30), (0.9, 45)):
        qq = q[4]
        k2 = keys([100.0, 104.0], [100.0, 100.0])
        d2 = descs(qq, [best, 50], rng)
        out.append(sfi_case("b", "ratio_%g_sfi" % ratio, keys([101.0], [100.0]), qq[None], k2, d2, win=10, ratio=ratio))
        out.append(points_case("b", "ratio_%g_points" % ratio, k2, d2, [(101.0, 100.0, 0, 0.9, qq, 1)], th=2.0, ratio=ratio))
        out.append(bow_case("b", "ratio_%g_bow" % ratio, keys([101.0], [100.0]), qq[None], [1], [4], k2, d2, [4, 4], ratio=ratio))
    # a single candidate at distance 40: the second-best stays at its initial value
    k2 = keys([100.0], [100.0])
    d2 = descs(q[5], [40], rng)
    out.append(sfi_case("b", "single_candidate_sfi", keys([101.0], [100.0]), q[5][None], k2, d2, win=10, ratio=0.9))
    out.append(points_case("b", "single_candidate_points", k2, d2, [(101.0, 100.0, 0, 0.9, q[5], 1)], th=2.0, ratio=0.9))
    return out


def family_c(rng):
    """Geometry: |dx| == r and r +- 1 ulp, half cells, x == maxX, negative coordinates, clamped and empty windows, nonzero
    minimum bounds."""
    out = []
    q = rand_desc(rng)[0]
    r = f32(10.0)
    up, dn = np.nextafter(r, f32(100)), np.nextafter(r, f32(0))
    k = keys([110.0, 100.0, 90.0, 100.0], [100.0, 110.0, 100.0, 90.0])
    area_q = [(100.0, 100.0, float(rr), -1, -1) for rr in (r, up, dn)]
    # half cells in float: (x - 0) * 0.1f lands on k + 0.5 for these x; x == maxX; negatives that round to 0 / -1
    hx = [105.0, 125.0, 5.0, 635.0, 640.0, -0.4, -5.0, 15.0, 320.0]
    hy = [105.0, 25.0, 475.0, 5.0, 240.0, 100.0, 100.0, -5.0, 480.0]
    kh = keys(hx, hy)
    out.append(_case("c", "grid_half_cells_and_edges", "grid", keys=kh, bounds=BOUNDS))
    edge_q = [(-50.0, 100.0, 10.0, -1, -1), (700.0, 100.0, 10.0, -1, -1), (100.0, -50.0, 10.0, -1, -1), (100.0, 530.0, 10.0, -1, -1),
              (0.0, 0.0, 30.0, -1, -1), (640.0, 480.0, 30.0, -1, -1), (-9.0, 240.0, 10.0, -1, -1), (649.0, 240.0, 10.0, -1, -1),
              (320.0, 240.0, 1000.0, -1, -1)]
    out.append(_case("c", "area_radius_and_edges", "area", keys=np.concatenate([k, kh]), bounds=BOUNDS, queries=area_q + edge_q))
    # the same radius edge through a matcher: th * mvScaleFactors[0] == 10 exactly, keypoint at dx == 10 and at dx == 10 - 1 ulp
    d = descs(q, [20, 30, 40, 50], rng)
    out.append(frame_case("c", "radius_edge_frame", k, d, [(100.0, 100.0, 0, 0.0, q, 1)], th=10.0, ori=False))
    kx = keys([float(f32(100.0) + dn), 110.0], [100.0, 100.0])
    out.append(frame_case("c", "radius_minus_ulp_frame", kx, descs(q, [30, 20], rng), [(100.0, 100.0, 0, 0.0, q, 1)], th=10.0, ori=False))
    # bounds as undistortion produces them (nonzero minimum): grid, area and SFI
    ub = (-12.5, 652.25, -8.75, 490.5)
    ku = keys([-12.5, -3.0, 652.25, 0.0, 320.0, 4.3125], [-8.75, 0.0, 490.5, 0.0, 240.0, 1.40625])
    out.append(_case("c", "grid_shifted_bounds", "grid", keys=ku, bounds=ub))
    out.append(_case("c", "area_shifted_bounds", "area", keys=ku, bounds=ub,
                     queries=[(-12.5, -8.75, 5.0, -1, -1), (652.25, 490.5, 3.0, -1, -1), (0.0, 0.0, 20.0, -1, -1), (-30.0, 240.0, 15.0, -1, -1)]))
    k1 = keys([-3.0, 0.5, 320.0], [0.5, 0.0, 240.0])
    out.append(sfi_case("c", "sfi_shifted_bounds", k1, np.stack([q, q, q]), ku, descs(q, [10, 20, 30, 12, 14, 44], rng), win=6, ratio=0.9, bounds=ub))
    # a keypoint right at maxX is outside the grid: no matcher can find it
    kmx = keys([640.0, 630.0], [100.0, 100.0])
    out.append(frame_case("c", "max_x_keypoint_frame", kmx, descs(q, [5, 40], rng), [(636.0, 100.0, 0, 0.0, q, 1)], th=10.0, ori=False))
    return out


def family_d(rng):
    """Levels: predicted level 0 (minLevel = -1) and the last level, F1 keypoints above level 0 in SFI, PredictScale clamped."""
    out = []
    q = rand_desc(rng)[0]
    k = keys([100.0, 102.0, 98.0, 300.0, 302.0, 298.0, 296.0], [100.0] * 3 + [300.0] * 4, octave=[0, 1, 2, 7, 6, 5, 8])
    d = descs(q, [30, 10, 5, 40, 20, 5, 3], rng)
    out.append(points_case("d", "level_0_and_last_points", k, d, [(100.0, 100.0, 0, 0.9, q, 1), (300.0, 300.0, 7, 0.9, q, 1)], th=1.0, ratio=0.9))
    out.append(frame_case("d", "level_0_and_last_frame", k, d, [(100.0, 100.0, 0, 0.0, q, 1), (300.0, 300.0, 7, 0.0, q, 1)], th=2.0, ori=False))
    out.append(_case("d", "area_levels", "area", keys=k, bounds=BOUNDS,
                     queries=[(100.0, 100.0, 10.0, -1, 0), (100.0, 100.0, 10.0, 0, 0), (100.0, 100.0, 10.0, 1, -1), (300.0, 300.0, 10.0, 6, 7),
                              (300.0, 300.0, 10.0, 6, 8), (300.0, 300.0, 10.0, -1, -1), (100.0, 100.0, 10.0, 0, -1)]))
    # SFI: F1 keypoints above level 0 are skipped, F2 keypoints above level 0 are not candidates
    k1 = keys([100.0, 100.0, 200.0], [100.0, 100.0, 200.0], octave=[1, 0, 2])
    k2 = keys([101.0, 102.0, 201.0], [100.0, 100.0, 200.0], octave=[1, 0, 0])
    out.append(sfi_case("d", "sfi_levels", k1, np.stack([q, q, q]), k2, descs(q, [2, 30, 3], rng), win=5, ratio=0.9))
    out.append(predict_scale_clamped_keyframe_case(rng))
    return out


def predict_scale_clamped_keyframe_case(rng):
    """Key-frame form: PredictScale clamped at 0 and at nlevels - 1, and on each level in between.  Every query has one
    keypoint per level (the higher the level, the closer the descriptor), so the predicted level decides the match.

    This case exposed a bug that the kernel and the oracle shared.  Upstream, the depth test compares dist3D with
    GetMin/MaxDistanceInvariance() = 0.8f*mfMinDistance / 1.2f*mfMaxDistance (ORBmatcher.cc:1519-1526, MapPoint.cc:390-400),
    but PredictScale divides the plain mfMaxDistance (MapPoint.cc:521).  The ABI took max_distance = 1.2f*mfMaxDistance
    and fed that same value to PredictScale, so the predicted level came out one too high.  It also made the lower clamp
    unreachable, since the depth test forced the ratio to be >= 1.  Upstream reaches it whenever
    mfMaxDistance < dist3D <= 1.2f*mfMaxDistance: the depths 9.5 / 12 with mfMaxDistance 9 / 10 below (ceil gives -0),
    and dist3D == 1.2f*4.81f exactly, where ceil gives -1 and the clamp itself acts; one ulp further the point is out of
    range.  The ABI now takes the plain mfMin/MaxDistance and forms 0.8f*min / 1.2f*max on the device."""
    q = rand_desc(rng)[0]
    kq, kk, kd = [], [], []
    depths = [(9.5, 9.0), (float(f32(f32(1.2) * f32(4.81))), 4.81), (12.0, 10.0), (10.0, 8.0), (1.0, 5000.0), (10.0, 10.0), (10.0, 12.0),
              (10.0, 12.000001), (10.0, 30.0), (2.0, 100.0), (10.0, 0.5), (float(np.nextafter(f32(f32(1.2) * f32(4.81)), f32(99))), 4.81)]
    for i, (dist3d, maxd) in enumerate(depths):
        x, y = _lattice(i + 20)
        mind = min(dist3d, maxd) * 0.5
        kq.append((x, y, dist3d, mind, maxd, 0.0, q, 0))
        for lv in range(8):
            kk.append((x + 1.0 + lv * 0.25, y + 0.5, lv))
            kd.append(90 - 10 * lv)
    karr = keys([a[0] for a in kk], [a[1] for a in kk], octave=[a[2] for a in kk])
    return keyframe_case("d", "predict_scale_clamped_keyframe", karr, descs(q, kd, rng), kq, th=3.0, orbdist=100, ori=False)


def _rot_spec(counts):
    """Rotation differences filling histogram bins: counts = {bin: n} -> list of rot values (deg) away from bin borders."""
    rots = []
    for b, n in sorted(counts.items()):
        rots += [30.0 * b + 3.0 * (j % 4) for j in range(n)]
    return rots


def _hist_cases(family, name, rots, rng, forms=("frame", "sfi", "bow", "keyframe"), ori=True):
    """One isolated keypoint per rotation value, every match at distance 10: the histogram alone decides what survives."""
    n = len(rots)
    xy = [_lattice(i) for i in range(n)]
    qd = rand_desc(rng, n)
    base = rng.uniform(0, 360, n).astype(np.float32)
    ka = np.zeros(n, np.float32)
    qa = np.zeros(n, np.float32)
    for i, rot in enumerate(rots):
        a, b = f32(base[i]), f32(rot)
        if rot == 0.0:
            qa[i], ka[i] = a, a
        elif rot < 0:                                               # a tiny negative difference: rot += 360
            qa[i], ka[i] = a, f32(a - b)
        else:
            qa[i], ka[i] = f32(a + b), a                            # rot = qa - ka (>= 360 wraps: still in range)
    k = keys([p[0] for p in xy], [p[1] for p in xy], angle=ka)
    d = np.array([at_distance(qd[i], 10, rng) for i in range(n)], np.uint8).reshape(-1, 32)
    out = []
    if "frame" in forms:
        out.append(frame_case(family, name + "_frame", k, d, [(xy[i][0] + 1.0, xy[i][1], 0, qa[i], qd[i], 1) for i in range(n)], th=5.0, ori=ori))
    if "keyframe" in forms:
        out.append(keyframe_case(family, name + "_keyframe", k, d, [(xy[i][0] + 1.0, xy[i][1], 4.0, 1.0, 4.0, qa[i], qd[i], 0) for i in range(n)],
                                 th=5.0, orbdist=50, ori=ori))
    if "sfi" in forms:
        k1 = keys([p[0] + 1.0 for p in xy], [p[1] for p in xy], angle=qa)
        out.append(sfi_case(family, name + "_sfi", k1, qd, k, d, win=5, ratio=0.9, ori=ori))
    if "bow" in forms:
        k1 = keys([p[0] for p in xy], [p[1] for p in xy], angle=qa)
        out.append(bow_case(family, name + "_bow", k1, qd, np.ones(n), np.arange(n) % 5, k, d, np.arange(n) % 5, ratio=0.9, ori=ori))
    return out


def family_e(rng):
    """The rotation histogram: rot 0, slightly negative, on and next to a half bin; count ties; the 0.1f rule at equality
    and one below, for max2 and max3; one bin; an empty histogram; checkOri off."""
    out = []
    out += _hist_cases("e", "tenth_equal_max2", _rot_spec({0: 10, 4: 1}), rng)             # 1 < 0.1f*10 is false: bin 4 kept
    out += _hist_cases("e", "tenth_below_max2", _rot_spec({0: 21, 4: 2}), rng, forms=("frame", "sfi"))      # 2 < 2.1: dropped
    out += _hist_cases("e", "tenth_float_max2", _rot_spec({1: 30, 5: 3}), rng, forms=("frame", "bow"))     # 0.1f*30 rounds to 3.0f
    out += _hist_cases("e", "tenth_equal_max3", _rot_spec({2: 30, 6: 10, 9: 3}), rng, forms=("frame", "keyframe"))
    out += _hist_cases("e", "tenth_below_max3", _rot_spec({0: 20, 1: 10, 2: 1}), rng, forms=("frame", "sfi"))
    out += _hist_cases("e", "count_ties", _rot_spec({1: 5, 3: 5, 5: 5, 7: 5, 11: 2}), rng)      # four equal bins: the earliest three
    out += _hist_cases("e", "count_ties_second", _rot_spec({0: 9, 4: 3, 8: 3, 12: 3}), rng, forms=("frame", "sfi"))
    out += _hist_cases("e", "one_bin", _rot_spec({6: 12}), rng, forms=("frame", "sfi"))
    out += _hist_cases("e", "ori_off", _rot_spec({0: 5, 3: 1, 6: 1, 9: 1, 12: 1}), rng, ori=False)
    h15 = f32(15.0)
    special = [0.0, 0.0, -1e-4, -2e-3, float(h15), float(h15), float(np.nextafter(h15, f32(0))), float(np.nextafter(h15, f32(30))),
               75.0, 75.0, 45.0, 30.0, 30.0, 60.0, 60.0, 90.0]
    out += _hist_cases("e", "half_bins", special, rng)
    # no match at all: the histogram stays empty
    q = rand_desc(rng)[0]
    k = keys([100.0, 300.0], [100.0, 300.0])
    out.append(frame_case("e", "empty_histogram_frame", k, descs(q, [120, 130], rng), [(100.0, 100.0, 0, 10.0, q, 1)], th=5.0))
    out.append(keyframe_case("e", "empty_histogram_keyframe", k, descs(q, [120, 130], rng), [(100.0, 100.0, 4.0, 1.0, 4.0, 10.0, q, 0),
                             (300.0, 300.0, 4.0, 1.0, 4.0, 10.0, q, 1), (-1.0, 100.0, 4.0, 1.0, 4.0, 10.0, q, 0)], th=5.0, orbdist=100))
    return out


def family_f(rng):
    """Conflicts: SFI steals on a strictly lower distance only; map points competing for one keypoint; occupied best candidates."""
    out = []
    q = rand_desc(rng, 4)
    k2 = keys([200.0, 205.0], [200.0, 200.0])
    d2 = np.stack([q[0], at_distance(q[0], 90, rng)])
    d1 = np.stack([at_distance(q[0], 30, rng), at_distance(q[0], 20, rng), at_distance(q[0], 20, rng), at_distance(q[0], 19, rng)])
    k1 = keys([200.0] * 4, [200.0] * 4, angle=[10.0, 20.0, 30.0, 40.0])
    out.append(sfi_case("f", "sfi_steal_lower_and_equal", k1, d1, k2, d2, win=20, ratio=0.9))
    # equal distance from a second keypoint that would otherwise have no candidate
    k1b = keys([200.0, 200.0, 400.0], [200.0, 200.0, 300.0])
    d1b = np.stack([at_distance(q[1], 25, rng)] * 2 + [q[2]])
    k2b = keys([201.0, 401.0], [200.0, 300.0])
    out.append(sfi_case("f", "sfi_equal_distance_blocked", k1b, d1b, k2b, np.stack([q[1], at_distance(q[2], 3, rng)]), win=10, ratio=0.9, ori=False))
    # points: a point without observations is overwritten, one with observations blocks the keypoint for later points
    k = keys([100.0, 103.0, 300.0, 303.0], [100.0, 100.0, 300.0, 300.0], octave=[0, 1, 0, 1])
    d = np.stack([q[3], at_distance(q[3], 30, rng), q[3], at_distance(q[3], 30, rng)])
    pq = [(101.0, 100.0, 1, 0.9, at_distance(q[3], 5, rng), 0), (101.0, 100.0, 1, 0.9, at_distance(q[3], 6, rng), 1),
          (101.0, 100.0, 1, 0.9, at_distance(q[3], 7, rng), 1), (301.0, 300.0, 1, 0.9, at_distance(q[3], 2, rng), 1),
          (301.0, 300.0, 1, 0.9, at_distance(q[3], 2, rng), 0)]
    out.append(points_case("f", "competing_points", k, d, pq, th=2.0, ratio=0.9))
    out.append(frame_case("f", "competing_points_frame", k, d, [(a, b, 0, 0.0, dd, o) for a, b, _, _, dd, o in pq], th=4.0, ori=True))
    kq = [(a, b, 4.0, 1.0, 4.0, 0.0, dd, 0) for a, b, _, _, dd, _ in pq]
    out.append(keyframe_case("f", "competing_points_keyframe", k, d, kq, th=4.0, orbdist=100, ori=False))
    # kp_has_point on the best candidate
    has = np.array([1, 0, 0, 1], np.uint8)
    out.append(points_case("f", "occupied_best_points", k, d, pq[1:4], th=2.0, ratio=0.9, has=has))
    out.append(frame_case("f", "occupied_best_frame", k, d, [(a, b, 0, 0.0, dd, o) for a, b, _, _, dd, o in pq], th=4.0, ori=False, has=has))
    out.append(keyframe_case("f", "occupied_best_keyframe", k, d, kq, th=4.0, orbdist=100, ori=False, has=has))
    # BoW: a later key-frame feature finds the best frame feature taken
    kk = keys([10.0, 20.0, 30.0], [10.0, 10.0, 10.0])
    fk = keys([10.0, 20.0], [10.0, 10.0])
    out.append(bow_case("f", "bow_taken", kk, np.stack([q[0], q[0], at_distance(q[0], 4, rng)]), [1, 1, 1], [2, 2, 2], fk,
                        np.stack([at_distance(q[0], 10, rng), at_distance(q[0], 40, rng)]), [2, 2], ratio=0.9, ori=False))
    return out


def _dense(n, rng, spread, center=(320.0, 240.0), octave=0):
    """n keypoints around `center`, indices in DEScending column order (cell order is the reverse of index order)."""
    xs = center[0] + rng.uniform(-spread, spread, n)
    ys = center[1] + rng.uniform(-spread, spread, n)
    o = np.argsort(-xs, kind="stable")
    return keys(xs[o].astype(np.float32), ys[o].astype(np.float32), octave=octave)


def _order(k, x, y, r, lo, hi, bounds=BOUNDS):
    return R.Grid(k, bounds).features_in_area(x, y, r, lo, hi)


def family_g(rng):
    """Capacity: 63 / 64 / 65 candidates and 319 / 320 / 321 (64 fixed slots + 256 pooled entries) with a tie across the limit,
    N = 0 and N = 1, every keypoint in one grid cell."""
    out = []
    for ncand in (63, 64, 65, 319, 320, 321, 400):
        q = rand_desc(rng)[0]
        k = _dense(ncand, rng, 25.0)
        cand = _order(k, 320.0, 240.0, 30.0, -1, 1)
        assert len(cand) == ncand
        lim = 64 if ncand < 100 else 320
        a, b = lim - 1, lim                                        # the tie straddles the limit (a == ncand - 1: last two)
        if b >= ncand:
            a, b = ncand - 2, ncand - 1
        dist = np.full(len(k), 80)
        dist[cand[a]], dist[cand[b]] = 40, 40
        d = descs(q, dist, rng)
        out.append(frame_case("g", "tie_at_%d_frame" % ncand, k, d, [(320.0, 240.0, 0, 0.0, q, 1)], th=30.0, ori=False))
        out.append(keyframe_case("g", "tie_at_%d_keyframe" % ncand, k, d, [(320.0, 240.0, 4.0, 1.0, 4.0, 0.0, q, 0)], th=30.0, ori=False))
        # points: alternate levels so the tie is accepted (different levels), the best at the limit
        k2 = k.copy()
        # (below 321 candidates the pair is the last two: inside the pool, the 63 / 64 / 65 cases straddle the fixed slots)
        k2["octave"] = np.arange(len(k)) % 2
        c2 = _order(k2, 320.0, 240.0, f32(f32(2.5 * 10.0) * SF[1]), 0, 1)
        assert c2 == cand                                          # levels do not change the candidate order
        d2 = np.full(len(k), 80)
        d2[c2[a]], d2[c2[b]] = 30, 30
        k2["octave"][c2[a]], k2["octave"][c2[b]] = 0, 1            # the tied pair on different levels: the ratio gate lets it pass
        out.append(points_case("g", "tie_at_%d_points" % ncand, k2, descs(q, d2, rng), [(320.0, 240.0, 1, 0.9995, q, 1)], th=10.0, ratio=0.9))
        # SFI: the unique best beyond the limit and the tie across it (rejected by the ratio test)
        d3 = np.full(len(k), 80)
        d3[cand[b]] = 20
        k1 = keys([320.0, 320.0], [240.0, 240.0])
        q2 = at_distance(q, 0, rng)
        d3b = np.full(len(k), 80)
        d3b[cand[a]], d3b[cand[b]] = 20, 20
        d2s = descs(q, d3, rng)
        d2b = descs(q2, d3b, rng)
        out.append(sfi_case("g", "best_at_%d_sfi" % ncand, k1[:1], q[None], k, d2s, win=30, ratio=0.9))
        out.append(sfi_case("g", "tie_at_%d_sfi" % ncand, k1[:1], q2[None], k, d2b, win=30, ratio=0.9))
    # more queries than fit the pool together: each query holds ~150 candidates, eight of them overlap
    q = rand_desc(rng, 8)
    k = _dense(500, rng, 60.0)
    dd = np.full(len(k), 90)
    qs = []
    for j in range(8):
        x, y = 280.0 + 10 * j, 240.0
        cand = _order(k, x, y, 40.0, -1, 1)
        dd[cand[-1]] = 20 + j
        qs.append((x, y, 0, 0.0, q[0], 1))
    out.append(frame_case("g", "overlapping_dense_queries_frame", k, descs(q[0], dd, rng), qs, th=40.0, ori=True))
    # N = 0 / N = 1
    e = keys([], [])
    ed = np.zeros((0, 32), np.uint8)
    q1 = rand_desc(rng)[0]
    out.append(frame_case("g", "n0_frame", e, ed, [(100.0, 100.0, 0, 0.0, q1, 1)], th=10.0))
    out.append(sfi_case("g", "n0_sfi_f2", keys([100.0], [100.0]), q1[None], e, ed, win=10))
    out.append(sfi_case("g", "n0_sfi_f1", e, ed, keys([100.0], [100.0]), q1[None], win=10))
    k1 = keys([100.0], [100.0])
    out.append(frame_case("g", "n1_frame", k1, descs(q1, [7], rng), [(100.0, 100.0, 0, 0.0, q1, 1), (100.0, 101.0, 0, 0.0, q1, 1)], th=10.0))
    out.append(points_case("g", "n1_points", k1, descs(q1, [7], rng), [(100.0, 100.0, 0, 0.9, q1, 1)], th=1.0))
    # every keypoint in one grid cell (cell 10 x 10 px): cell order == insertion order, and 70 candidates
    k = keys(rng.uniform(195.5, 204.4, 70).astype(np.float32), rng.uniform(195.5, 204.4, 70).astype(np.float32))
    dist = rng.randint(30, 60, 70)
    dist[[5, 66]] = 10
    out.append(_case("g", "one_cell_grid", "grid", keys=k, bounds=BOUNDS))
    out.append(frame_case("g", "one_cell_frame", k, descs(q1, dist, rng), [(200.0, 200.0, 0, 0.0, q1, 1)], th=20.0, ori=False))
    out.append(sfi_case("g", "one_cell_sfi", keys([200.0], [200.0]), q1[None], k, descs(q1, np.where(dist == 10, 70, dist), rng), win=20))
    return out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}
# the edges each family must reach (matcher_reference counts them)
TARGETS = {
    "a": ("tie_best", "area_order_not_index", "ratio_gate_same_level", "ratio_gate_other_level"),
    "b": ("threshold_edge", "ratio_boundary", "single_candidate"),
    "c": ("area_on_radius", "grid_half_cell", "grid_rejected", "area_empty_left", "area_empty_right", "area_empty_top", "area_empty_bottom"),
    "d": ("area_level_floor_open", "sfi_skipped_level", "predicted_level_first", "predicted_level_last", "predict_ratio_below_one",
          "predict_scale_clamped_low"),
    "e": ("rot_half_bin", "rot_negative", "hist_count_tie", "hist_tenth_equal"),
    "f": ("sfi_steal", "sfi_equal_to_taken", "overwrite_without_observations", "candidate_blocked"),
    "g": ("area_over_64", "area_over_320"),
}


def all_cases(seed=0, families="abcdefg"):
    rng = np.random.RandomState(seed)
    out = []
    for f in families:
        out += FAMILIES[f](rng)
    return out


# ---------------------------------------------------------------- running a case
def _log_sf():
    return f32(R.contract_log_f()(SF[1]))


def run_reference(case, rules=R.REFERENCE, hits=None):
    a, kind = case["a"], case["kind"]
    if kind == "grid":
        return R.Grid(a["keys"], a["bounds"], rules, hits).csr()
    if kind == "area":
        g = R.Grid(a["keys"], a["bounds"], rules, hits)
        return [np.array(g.features_in_area(*qq, hits=hits), np.int32) for qq in a["queries"]]
    if kind == "sfi":
        return R.search_for_initialization(a["k1"], a["d1"], a["k2"], a["d2"], a["bounds"], a["prev"], a["win"], a["ratio"], a["ori"], rules, hits)
    if kind == "points":
        return R.search_by_projection_points(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["px"], a["py"], a["lvl"], a["vc"],
                                             a["pd"], a["obs"], a["th"], a["ratio"], rules, hits)
    if kind == "frame":
        return R.search_by_projection_frame(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["u"], a["v"], a["oct"], a["ang"],
                                            a["pd"], a["obs"], a["th"], a["ori"], rules, hits)
    if kind == "keyframe":
        return R.search_by_projection_keyframe(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["found"], a["u"], a["v"], a["d3"],
                                               a["mind"], a["maxd"], _log_sf(), a["ang"], a["pd"], a["th"], a["orbdist"], a["ori"],
                                               rules=rules, hits=hits)
    if kind == "bow":
        return R.search_by_bow(a["kd"], a["kk"]["angle"], a["kv"], a["kfv"], a["fd"], a["fk"]["angle"], a["ffv"], a["ratio"], a["ori"], rules, hits)
    raise ValueError(kind)


def run_oracle(case, oracle):
    a, kind = case["a"], case["kind"]
    if kind == "grid":
        return oracle.frame_grid(a["keys"], a["bounds"])
    if kind == "area":
        g = oracle.frame_grid(a["keys"], a["bounds"])
        gg = (g[0], np.concatenate([g[1], np.zeros(1, np.int32)]))
        return [oracle.features_in_area(a["keys"], gg, a["bounds"], *qq) for qq in a["queries"]]
    if kind == "sfi":
        return oracle.search_for_initialization(a["k1"], a["d1"], a["k2"], a["d2"], a["bounds"], a["prev"], a["win"], a["ratio"], a["ori"])
    if kind == "points":
        return oracle.search_by_projection_points(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["px"], a["py"], a["lvl"], a["vc"],
                                                  a["pd"], a["obs"], a["th"], a["ratio"])
    if kind == "frame":
        return oracle.search_by_projection_frame(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["u"], a["v"], a["oct"], a["ang"],
                                                 a["pd"], a["obs"], a["th"], a["ori"])
    if kind == "keyframe":
        return oracle.search_by_projection_keyframe(a["keys"], a["desc"], a["bounds"], SF, a["has"], a["valid"], a["found"], a["u"], a["v"],
                                                    a["d3"], a["mind"], a["maxd"], _log_sf(), a["ang"], a["pd"], a["th"], a["orbdist"], a["ori"])
    if kind == "bow":
        return oracle.search_by_bow(a["kd"], a["kk"]["angle"], a["kv"], a["kfv"], a["fd"], a["fk"]["angle"], a["ffv"], a["ratio"], a["ori"])
    raise ValueError(kind)


def same(x, y):
    """Results equal bit for bit (tuples / lists of arrays and ints)."""
    if isinstance(x, (tuple, list)):
        return isinstance(y, (tuple, list)) and len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        x, y = np.asarray(x), np.asarray(y)
        return x.shape == y.shape and x.tobytes() == y.tobytes()
    return int(x) == int(y)


def _family_ids():
    return list(FAMILIES)


# ---------------------------------------------------------------- GPU: single calls and batched device forms
class ArrayFrame:
    """A Frame built from arrays (what pg.Frame holds after extraction): mvKeys, mDescriptors, bounds, the device grid."""

    def __init__(self, ext, k, d, bounds):
        self.ext = ext
        self.mvKeys = self.mvKeysUndistorted = np.ascontiguousarray(k, KEYPOINT_DTYPE)
        self.mDescriptors = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
        self.N = len(k)
        self.bounds = tuple(float(b) for b in bounds)
        self.grid_start = np.zeros(64 * 48 + 1, np.int32)
        self.grid_idx = np.zeros(max(self.N, 1), np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        ext._check(ext._L.pgorb_frame_grid(ext._h, p(self.mvKeys), self.N, *self.bounds, p(self.grid_start), p(self.grid_idx)))


def run_gpu(case, ext):
    import pilotguru_amd as pg
    a, kind = case["a"], case["kind"]
    if kind == "grid":
        F = ArrayFrame(ext, a["keys"], np.zeros((len(a["keys"]), 32), np.uint8), a["bounds"])
        return F.grid_start, F.grid_idx[:F.grid_start[-1]].copy()
    if kind == "sfi":
        F1, F2 = ArrayFrame(ext, a["k1"], a["d1"], a["bounds"]), ArrayFrame(ext, a["k2"], a["d2"], a["bounds"])
        prev = a["prev"].copy()
        nm, m12 = pg.ORBmatcher(a["ratio"], a["ori"]).SearchForInitialization(F1, F2, prev, a["win"])
        return nm, m12, prev
    if kind == "points":
        F = ArrayFrame(ext, a["keys"], a["desc"], a["bounds"])
        mp = pg.MapPoints(a["valid"], a["px"], a["py"], a["lvl"], a["vc"], a["pd"], a["obs"])
        return pg.ORBmatcher(a["ratio"], True).SearchByProjection(F, mp, a["th"], a["has"])
    if kind == "frame":
        F = ArrayFrame(ext, a["keys"], a["desc"], a["bounds"])
        return pg.ORBmatcher(0.9, a["ori"]).SearchByProjectionLastFrame(F, a["valid"], a["u"], a["v"], a["oct"], a["ang"], a["pd"], a["obs"],
                                                                        a["th"], a["has"])
    if kind == "keyframe":
        F = ArrayFrame(ext, a["keys"], a["desc"], a["bounds"])
        return pg.ORBmatcher(0.9, a["ori"]).SearchByProjectionKeyFrame(F, a["valid"], a["found"], a["u"], a["v"], a["d3"], a["mind"], a["maxd"],
                                                                       a["ang"], a["pd"], a["th"], a["orbdist"], a["has"])
    if kind == "bow":
        F = ArrayFrame(ext, a["fk"], a["fd"], BOUNDS)
        return pg.ORBmatcher(a["ratio"], a["ori"]).SearchByBoW(ext, a["kd"], a["kk"]["angle"], a["kv"], a["kfv"], F, a["ffv"])
    return None


def _pack_frames(frames, extra, poison):
    """Frames (keys, desc) into the pgorb_extract_batch_device layout: cap = largest n + extra, slots past n poisoned."""
    import torch
    B = len(frames)
    cap = max([len(k) for k, _ in frames] + [1]) + extra
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    for f, (k, d) in enumerate(frames):
        n = len(k)
        kp[f, :n] = k
        if poison == "nan":
            kp[f, n:]["x"], kp[f, n:]["y"] = np.nan, np.nan
        else:
            kp[f, n:]["x"], kp[f, n:]["y"] = 3.0e38, -3.0e38
        kp[f, n:]["octave"] = 0
        ds[f, :n] = d
    n = np.array([len(k) for k, _ in frames], np.int32)
    dk = torch.from_numpy(kp.view(np.uint8).reshape(B, cap, 28).copy()).cuda()
    return dk, torch.from_numpy(ds).cuda(), torch.from_numpy(n).cuda(), cap


def run_gpu_batched(cases, ext, poison, extra=7, qextra=3):
    """Every case of one kind in one launch of the *_batch_device form; returns the per-case results.  cap = the largest
    frame + extra, qcap = the longest query list + qextra (tests/capacity_cases.py passes 0: the caps themselves are the case)."""
    import torch
    L, h = ext._L, ext._h
    keep = []                                   # device tensors stay referenced until the launch has finished

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kind = cases[0]["kind"]
    A = [c["a"] for c in cases]
    if kind == "sfi":
        frames = [(a["k1"], a["d1"]) for a in A] + [(a["k2"], a["d2"]) for a in A]
        bounds = A[0]["bounds"]
    elif kind == "bow":
        frames = [(a["kk"], a["kd"]) for a in A] + [(a["fk"], a["fd"]) for a in A]
        bounds = BOUNDS
    else:
        frames = [(a["keys"], a["desc"]) for a in A]
        bounds = A[0]["bounds"]
    B, P = len(frames), len(cases)
    dk, dd, dn, cap = _pack_frames(frames, extra, poison)
    gs = torch.empty((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    gi = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(h, p(dk), p(dn), B, cap, *bounds, p(gs), p(gi), s))
    torch.cuda.synchronize()
    grids = [(gs[f].cpu().numpy(), gi[f, :int(gs[f, -1])].cpu().numpy()) for f in range(B)]
    asg = torch.full((P, cap), -9, dtype=torch.int32, device="cuda")
    nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    pair = torch.arange(P, dtype=torch.int32, device="cuda")
    if kind == "sfi":
        prev = np.zeros((P, cap, 2), np.float32)
        for j, a in enumerate(A):
            prev[j, :len(a["prev"])] = a["prev"]
        dprev = torch.from_numpy(prev).cuda()
        ext._check(L.pgorb_search_for_initialization_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pair), p(pair + P), P, *bounds,
                                                                 p(dprev), p(asg), p(nm), A[0]["win"], A[0]["ratio"], int(A[0]["ori"]), s))
        torch.cuda.synchronize()
        res = [(int(nm[j]), asg[j, :len(a["k1"])].cpu().numpy(), dprev[j, :len(a["k1"])].cpu().numpy()) for j, a in enumerate(A)]
        return grids, res
    if kind == "bow":
        fvn = np.zeros((B, cap), np.uint32); fvs = np.zeros((B, cap + 1), np.int32); fvf = np.zeros((B, cap), np.uint32)
        nfv = np.zeros(B, np.int32)
        for f, fv in enumerate([a["kfv"] for a in A] + [a["ffv"] for a in A]):
            nfv[f] = len(fv[0]); fvn[f, :len(fv[0])] = fv[0]; fvs[f, :len(fv[1])] = fv[1]; fvf[f, :len(fv[2])] = fv[2]
        kv = np.zeros((P, cap), np.uint8)
        for j, a in enumerate(A):
            kv[j, :len(a["kv"])] = a["kv"]
        T = lambda x: torch.from_numpy(x).cuda()
        ext._check(L.pgorb_search_by_bow_batch_device(h, p(dk), p(dd), p(dn), cap, p(T(fvn)), p(T(fvs)), p(T(fvf)), p(T(nfv)), p(pair),
                                                     p(pair + P), P, p(T(kv)), A[0]["ratio"], int(A[0]["ori"]), p(asg), p(nm), s))
        torch.cuda.synchronize()
        return grids, [(int(nm[j]), asg[j, :len(a["fk"])].cpu().numpy()) for j, a in enumerate(A)]
    qcap = max(len(a["valid"]) for a in A) + qextra

    def qpack(key, dtype, width=None):
        x = np.zeros((P, qcap) + ((width,) if width else ()), dtype)
        for j, a in enumerate(A):
            x[j, :len(a[key])] = a[key]
        return torch.from_numpy(x).cuda()
    has = np.zeros((P, cap), np.uint8)
    for j, a in enumerate(A):
        has[j, :len(a["has"])] = a["has"]
    dhas = torch.from_numpy(has).cuda()
    nq = torch.tensor([len(a["valid"]) for a in A], dtype=torch.int32, device="cuda")
    if kind == "points":
        ext._check(L.pgorb_search_by_projection_points_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pair), P, *bounds, p(dhas), qcap,
                   p(nq), p(qpack("valid", np.uint8)), p(qpack("px", np.float32)), p(qpack("py", np.float32)), p(qpack("lvl", np.int32)),
                   p(qpack("vc", np.float32)), p(qpack("pd", np.uint8, 32)), p(qpack("obs", np.uint8)), A[0]["th"], A[0]["ratio"], p(asg), p(nm), s))
    elif kind == "frame":
        ext._check(L.pgorb_search_by_projection_frame_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pair), P, *bounds, p(dhas), qcap,
                   p(nq), p(qpack("valid", np.uint8)), p(qpack("u", np.float32)), p(qpack("v", np.float32)), p(qpack("oct", np.int32)),
                   p(qpack("ang", np.float32)), p(qpack("pd", np.uint8, 32)), p(qpack("obs", np.uint8)), A[0]["th"], int(A[0]["ori"]), p(asg), p(nm), s))
    elif kind == "keyframe":
        ext._check(L.pgorb_search_by_projection_keyframe_batch_device(h, p(dk), p(dd), p(dn), cap, p(gs), p(gi), p(pair), P, *bounds, p(dhas), qcap,
                   p(nq), p(qpack("valid", np.uint8)), p(qpack("found", np.uint8)), p(qpack("u", np.float32)), p(qpack("v", np.float32)),
                   p(qpack("d3", np.float32)), p(qpack("mind", np.float32)), p(qpack("maxd", np.float32)), p(qpack("ang", np.float32)),
                   p(qpack("pd", np.uint8, 32)), ext.log_scale_factor(), A[0]["th"], A[0]["orbdist"], int(A[0]["ori"]), p(asg), p(nm), s))
    torch.cuda.synchronize()
    return grids, [(int(nm[j]), asg[j, :len(a["keys"])].cpu().numpy()) for j, a in enumerate(A)]


def run_gpu_grid_batched(cases, ext, poison):
    """Grid cases of one bounds rectangle through pgorb_frame_grid_batch_device in one launch (poisoned slots past n)."""
    import torch
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bounds = cases[0]["a"]["bounds"]
    frames = [(c["a"]["keys"], np.zeros((len(c["a"]["keys"]), 32), np.uint8)) for c in cases]
    dk, dd, dn, cap = _pack_frames(frames, 5, poison)
    B = len(frames)
    gs = torch.full((B, 64 * 48 + 1), -3, dtype=torch.int32, device="cuda")
    gi = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(dk), p(dn), B, cap, *bounds, p(gs), p(gi), s))
    torch.cuda.synchronize()
    return [(gs[f].cpu().numpy(), gi[f, :int(gs[f, -1])].cpu().numpy()) for f in range(B)]


def grid_groups(cases):
    """Grid cases grouped by bounds (one batched launch each)."""
    groups = collections.OrderedDict()
    for c in cases:
        if c["kind"] == "grid":
            groups.setdefault(tuple(c["a"]["bounds"]), []).append(c)
    return list(groups.values())


def _batch_groups(cases):
    """Cases that can share one batched launch: same kind and the same scalar parameters."""
    groups = collections.OrderedDict()
    for c in cases:
        a = c["a"]
        if c["kind"] in ("grid", "area"):
            continue
        key = (c["kind"], tuple(a.get("bounds", BOUNDS)), a.get("th"), a.get("ratio"), a.get("ori"), a.get("win"), a.get("orbdist"))
        groups.setdefault(key, []).append(c)
    return list(groups.values())


def _case_frames(case):
    a = case["a"]
    if case["kind"] == "sfi":
        return [(a["k1"], a["bounds"]), (a["k2"], a["bounds"])]
    if case["kind"] == "bow":
        return [(a["kk"], BOUNDS), (a["fk"], BOUNDS)]
    return [(a["keys"], a["bounds"])]
