"""The constructed two-view scenes of tests/test_initializer.py: 640 x 480, fx = fy = 500, each built for one property of
Initializer::Initialize (tests/init_reference.py) and checked for it by test_cases_reach_what_they_are_built_for.

A scene is a set of 3-D points in the frame of the first camera (depth 4 - 9), seen by a second camera x2 = R*x1 + t, with pixel
noise and a share of outliers (a match to a random pixel).  The matched keypoints sit at rising indices among the keypoints of
frame 1 and at shuffled indices in frame 2; the others are unmatched.  Every random choice comes from a RandomState seeded per case.
"""
import os
import types
import zlib

import numpy as np

from tests import init_reference as IR

f32, f64 = np.float32, np.float64
W, H = 640, 480
CAMERA = np.array([500, 500, 320, 240, 1 / 500, 1 / 500], f32)          # fx, fy, cx, cy, invfx, invfy
ROTATION = (0.02, -0.05, 0.01)
BASELINE = (0.5, 0.05, 0.1)
DEFAULTS = dict(sigma=1.0, iters=24, min_parallax=1.0, min_tri=50)
SPREAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_spread.json")
ULPS = 64                                                                 # the condition on the parallax (see `condition`)


def rodrigues(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def project(X):
    return np.stack([500.0 * X[:, 0] / X[:, 2] + 320.0, 500.0 * X[:, 1] / X[:, 2] + 240.0], 1)


def backproject(uv, z):
    return np.stack([(uv[:, 0] - 320.0) / 500.0 * z, (uv[:, 1] - 240.0) / 500.0 * z, z], 1)


def draws_for_set(sel, N):
    """raw rand() values that make the swap-with-back selection pick `sel` (8 distinct indices below N)"""
    avail = list(range(N))
    out = []
    for want in sel:
        r = avail.index(want)
        out.append(int((r + 0.5) * 2147483648.0 / len(avail)))
        avail[r] = avail[-1]
        avail.pop()
    assert IR.select_list(out, N) == list(sel)
    return out


def scene(name, N, kind="general", outliers=0.2, noise=0.3, extra1=0, extra2=0, far=False, gaps=0, behind=0, rot=ROTATION, base=BASELINE,
          collinear=0, twins=0, same8=False, zero_u1=False, column1=False, sets=None, **params):
    """kind: general | planar | identical.  extra1 / extra2: unmatched keypoints (far: in a corner away from the matched ones).
    gaps: runs of unmatched keypoints inside frame 1's list.  behind: that many matches whose frame-2 point is the projection of
    a point BEHIND camera 1 on the same ray (it satisfies the epipolar constraint and triangulates to a negative depth).
    collinear: the first `collinear` matched points of frame 1 lie on one image line.  twins: the second correspondence repeats the
    first (two keypoints with the same coordinates in each frame).  same8: the first eight correspondences are one and the same.
    zero_u1: frame 1 in integer pixels, the first eight matched points at x = 300 and the frame's mean x exactly 300, so their
    normalised u1 is exactly 0: three rows of ComputeH21's A^T vanish, vt.row(8) is a unit vector and H21i is exactly singular.
    column1: every keypoint of frame 1 at x = 300, so meanDevX is 0, sX is infinite and every hypothesis of both models is NaN.
    sets: {iteration: [8 match indices] | "zeros" | "max"} fixes that iteration's draws."""
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    c = types.SimpleNamespace(name=name, N=N, kind=kind)
    R, t = rodrigues(rot), np.asarray(base, f64)
    uv1 = rng.uniform([40, 40], [W - 40, H - 40], (N, 2))
    if collinear:
        uv1[:collinear, 1] = 100.0 + 0.25 * (uv1[:collinear, 0] - 40.0)
    if kind == "planar":
        z = 1.0 / (1.0 / 6.0 + 1e-4 * (uv1[:, 0] - 320.0) + 5e-5 * (uv1[:, 1] - 240.0))   # a plane: 1/z is affine in the pixel
    else:
        z = rng.uniform(4.0, 9.0, N)
    X = backproject(uv1, z)
    if kind == "identical":
        uv2 = uv1.copy()
    else:
        uv2 = project(X @ R.T + t)
        if behind:
            b = rng.permutation(N)[:behind]
            uv2[b] = project((-X[b]) @ R.T + t)
            c.behind = np.sort(b)
        uv1 = uv1 + rng.normal(size=(N, 2)) * noise
        uv2 = uv2 + rng.normal(size=(N, 2)) * noise
    good = np.ones(N, bool)
    nout = int(round(outliers * N))
    if nout:
        o = rng.permutation(np.arange(max(collinear, 8 if same8 else 0, 2 if twins else 0), N))[:nout]
        uv2[o] = rng.uniform([0, 0], [W, H], (nout, 2))
        good[o] = False
    if twins:
        uv1[1], uv2[1] = uv1[0], uv2[0]
    if same8:
        uv1[:8], uv2[:8] = uv1[0], uv2[0]
    if column1 or zero_u1:                                             # integer pixels: frame 1's float sums are exact
        uv1 = np.round(uv1)
    if column1:
        uv1[:, 0] = 300.0
    if zero_u1:
        uv1[:8, 0] = 300.0
    n1, n2 = N + extra1 + gaps, N + extra2

    def others(k):
        return rng.uniform([2, 2], [30, 30], (k, 2)) if far else rng.uniform([0, 0], [W, H], (k, 2))
    k1, k2 = others(n1), others(n2)
    slot1 = np.sort(rng.permutation(n1 - gaps)[:N])
    if gaps:                                                            # a run of `gaps` unmatched keypoints after the first third
        slot1 = np.where(np.arange(N) >= N // 3, slot1 + gaps, slot1)
    slot2 = rng.permutation(n2)[:N]
    k1[slot1], k2[slot2] = uv1, uv2
    if column1:
        k1[:, 0] = 300.0
    if zero_u1:                                                         # one unmatched keypoint brings the frame's mean x to exactly 300
        k1 = np.round(k1)
        free = np.setdiff1d(np.arange(n1), slot1)[0]
        k1[free, 0] = 300.0 * n1 - (k1[:, 0].sum() - k1[free, 0])
    c.k1, c.k2 = k1.astype(f32), k2.astype(f32)
    c.matches12 = np.full(n1, -1, np.int32)
    c.matches12[slot1] = slot2
    c.good, c.R, c.t, c.X = good, R, t, X
    c.camera = CAMERA
    c.params = dict(DEFAULTS, **params)
    it = c.params["iters"]
    c.draws = rng.randint(0, 2 ** 31, (it, 8)).astype(np.uint32)
    for k, s in (sets or {}).items():
        if isinstance(s, str):
            c.draws[k] = 0 if s == "zeros" else 2 ** 31 - 1
        else:
            c.draws[k] = draws_for_set(list(s), N)
    return c


def run(c, mut=(), form="window"):
    p = c.params
    return IR.initialize(c.k1, c.k2, c.camera, c.matches12, p["sigma"], p["iters"], p["min_parallax"], p["min_tri"], c.draws, mut=mut, form=form)


def build():
    S = scene
    g8 = list(range(8))
    return [
        S("few_7", 7, outliers=0),
        S("n8_all", 8, outliers=0, iters=6),
        S("n9", 9, outliers=0, iters=6),
        S("n63", 63), S("n64", 64), S("n65", 65), S("n257", 257),
        S("planar_64", 64, "planar"), S("planar_120", 120, "planar"), S("planar_257", 257, "planar"),
        S("general_ok", 80, outliers=0.1, noise=0.05, extra1=7, extra2=3),
        S("general_200", 70, outliers=0.2, iters=200),
        S("rotation_only", 100, base=(0, 0, 0)),
        S("tiny_baseline", 100, base=(0.01, 0.001, 0.002)),
        S("identical", 90, "identical", outliers=0),
        S("uneven_frames", 72, extra1=41, extra2=17, far=True),
        S("gaps", 66, gaps=29, extra1=5),
        S("collinear_set", 64, collinear=8, sets={0: g8, 1: "zeros", 2: "max"}),
        S("twin_set", 64, twins=1, sets={0: g8}),
        S("same8_set", 64, same8=True, sets={0: g8}, outliers=0.1),
        S("good_50", 50, outliers=0, noise=0.05), S("good_51", 51, outliers=0, noise=0.05), S("good_52", 52, outliers=0, noise=0.05),
        S("planar_good_50", 50, "planar", outliers=0, noise=0.05), S("planar_good_51", 51, "planar", outliers=0, noise=0.05),
        S("ninety_percent", 60, outliers=0, noise=0.05, behind=6),
        S("behind_half", 80, outliers=0, noise=0.05, behind=34),
        S("one_iteration", 40, outliers=0, iters=1),
        S("singular_h", 64, zero_u1=True, extra1=3, sets={0: g8}),
        S("no_model", 30, column1=True, extra1=2, iters=3),
    ]


def parallax_tolerance(value, spread):
    """the larger of 2 float ulps at the value and 16 times the recorded spread of the reference's own acos forms"""
    return max(2.0 * float(np.spacing(f32(abs(value)))), 16.0 * spread)


def spread(c, out):
    """the largest difference among the three acos forms over the order statistics of this case's hypotheses"""
    s = 0.0
    for cs in out.get("cosines", []):
        if cs:
            a = [float(x) for x in IR.parallax_forms(cs[min(50, len(cs) - 1)])]
            s = max(s, max(a) - min(a))
    return s


def condition(c, out):
    """What makes every decision comparable exactly: RH is not within 0.02 of 0.40, no parallax is within ULPS float ulps of
    min_parallax, and no cosine that CheckRT sorts is a NaN.  Returns the list of violations."""
    bad = []
    st = int(out["info"][IR.I_STATUS])
    if st & (IR.MODEL_H | IR.MODEL_F):
        rh = float(out["finfo"][IR.F_RH])
        if abs(rh - 0.40) < 0.02:
            bad.append("RH %.4f" % rh)
    mp = f32(c.params["min_parallax"])
    for i, cs in enumerate(out.get("cosines", [])):
        if any(x != x for x in cs):
            bad.append("a NaN cosine in hypothesis %d" % i)
        if cs:
            p = out["finfo"][IR.F_PARALLAX + i]
            if abs(float(p) - float(mp)) <= ULPS * float(np.spacing(mp)):
                bad.append("parallax %r of hypothesis %d" % (p, i))
    return bad


def _hyp(tr, k):
    """hypothesis k of a trace (the reference's list of dicts, or an INIT_HYPOTHESIS_DTYPE array) as comparable pieces"""
    h = tr[k]
    if isinstance(h, dict):
        return (np.array(h["H21"] + h["F21"] + [h["scoreH"], h["scoreF"]], f32), [sum(h["inlH"]), sum(h["inlF"])] + list(h["set"]))
    return (np.concatenate([h["H21"], h["F21"], [h["scoreH"], h["scoreF"]]]).astype(f32),
            [int(h["inliersH"]), int(h["inliersF"])] + [int(x) for x in h["set"]])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32).ravel(), np.ascontiguousarray(b, f32).ravel()
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def differences(a, b, spread, exact_parallax=False):
    """the names of the outputs in which two results differ: every traced hypothesis and every other output byte for byte (a NaN
    equals a NaN), the parallaxes of finfo within parallax_tolerance (exact_parallax: bit for bit as well)"""
    bad = []
    if len(a["trace"]) != len(b["trace"]):
        bad.append("trace length")
    else:
        for k in range(len(a["trace"])):
            (fa, ia), (fb, ib) = _hyp(a["trace"], k), _hyp(b["trace"], k)
            if not _same_bits(fa, fb) or ia != ib:
                bad.append("hypothesis %d" % k)
    for k in ("pose", "P3D", "points"):
        if k in a and k in b and not _same_bits(a[k], b[k]):
            bad.append(k)
    for k in ("triangulated", "matches12_out", "kf_point1", "kf_point2", "obs_start", "obs_frame", "obs_idx", "info"):
        if k in a and k in b and not np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)):
            bad.append(k)
    if int(a["ret"]) != int(b["ret"]) or ("npoints" in a and "npoints" in b and int(a["npoints"]) != int(b["npoints"])):
        bad.append("count")
    fa, fb = np.asarray(a["finfo"], f32), np.asarray(b["finfo"], f32)
    if not _same_bits(fa[:IR.F_PARALLAX], fb[:IR.F_PARALLAX]):
        bad.append("SH, SF, RH")
    for i in range(IR.F_PARALLAX, IR.FINFO):
        x, y = float(fa[i]), float(fb[i])
        if (x != x) != (y != y) or (x == x and (x != y if exact_parallax else abs(x - y) > parallax_tolerance(x, spread))):
            bad.append("parallax %d" % (i - IR.F_PARALLAX))
    return bad
