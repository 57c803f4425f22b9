"""Constructed edge cases of SearchForTriangulation (pilotguru_amd/csrc/node_match.hip, k_search_for_triangulation) and the runners that
put them through the plain reference (tests/triangulation_reference.py), the single-call ABI and the batched device form.
A helper module (no tests): tests/test_search_for_triangulation.py uses it.

Key frames are built straight from arrays, with descriptors at exact Hamming distances from their queries and every
candidate's place relative to the epipolar line and the epipole chosen.  Most cases use F_H, the fundamental matrix of a pure
sideways translation ([t]x with t = (1, 0, 0)): the epipolar line of (x1, y1) is y = y1, so a candidate at (x, y1 + e) lies
e px off its line; the epipole is far away unless a case places it."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulation_reference as T  # noqa: E402
from matcher_cases import SF, _fv, descs, keys, rand_desc  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE  # noqa: E402

f32 = np.float32
S2 = T.level_sigma2(SF)
F_H = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
EP_FAR = (-1.0e4, -1.0e4)


def case(name, k1, d1, node1, k2, d2, node2, F=F_H, ep=EP_FAR, ori=True, h1=None, h2=None):
    n1, n2 = len(k1), len(k2)
    return dict(name=name, k1=k1, d1=np.asarray(d1, np.uint8).reshape(-1, 32), fv1=_fv(node1),
                h1=np.zeros(n1, np.uint8) if h1 is None else np.asarray(h1, np.uint8),
                k2=k2, d2=np.asarray(d2, np.uint8).reshape(-1, 32), fv2=_fv(node2),
                h2=np.zeros(n2, np.uint8) if h2 is None else np.asarray(h2, np.uint8),
                F=np.asarray(F, np.float32).reshape(3, 3), ep=(f32(ep[0]), f32(ep[1])), ori=bool(ori))


def _one_query(name, dists, offsets, rng, octave=0, ep=EP_FAR, h2=None, ori=True, x0=200.0):
    """KF1 keypoint (100, 100) against KF2 candidates in one node, in list order: at (x0 + 20 k, 100 + offsets[k]), offsets[k] px
    off the epipolar line, at Hamming distance dists[k]."""
    q = rand_desc(rng)[0]
    k1 = keys([100.0], [100.0])
    xs = [x0 + 20.0 * k for k in range(len(dists))]
    k2 = keys(xs, [100.0 + o for o in offsets], octave=octave)
    return case(name, k1, q[None], [3], k2, descs(q, dists, rng), [3] * len(dists), ep=ep, h2=h2, ori=ori)


def _float_search(start, pred, steps=4000):
    """The float nearest `start` (walking down) for which pred holds."""
    cur = f32(start)
    for _ in range(steps):
        if pred(cur):
            return cur
        cur = np.nextafter(cur, f32(-np.inf), dtype=np.float32)
    raise AssertionError("no float found below %r" % start)


def family_threshold(rng):
    return [_one_query("dist 50 kept", [51, 50], [0, 0], rng),
            _one_query("dist 51 never kept", [51], [0], rng),
            _one_query("dist 50 alone", [50], [0], rng)]


def family_ties(rng):
    out = [_one_query("equal distances: the later passing one wins", [30, 30], [0, 0.5], rng),
           _one_query("equal distances: the later one fails the line", [30, 30], [0, 3.0], rng),
           _one_query("closer candidate fails the line, bestDist stays", [20, 30], [5.0, 0], rng),
           _one_query("closer candidate fails the epipole test", [20, 30], [0, 0], rng, ep=(200.0, 103.0))]
    # ties across lanes and register slots of a 200-candidate node
    q = rand_desc(rng)[0]
    dists = [128] * 200
    dists[70], dists[190], dists[5] = 12, 12, 40
    k2 = keys([1.0 + 3.0 * k for k in range(200)], [100.0] * 200)
    out.append(case("tie across register slots (positions 70, 190)", keys([50.0], [100.0]), q[None], [9], k2, descs(q, dists, rng), [9] * 200))
    # two KF1 keypoints take the same KF2 keypoint (vbMatched2 never set)
    q1 = rand_desc(rng)[0]
    d1 = np.stack([q1, descs(q1, [10], rng)[0]])
    out.append(case("two KF1 keypoints share one KF2 keypoint", keys([100.0, 140.0], [100.0, 100.0]), d1, [4, 4],
                    keys([300.0], [100.0]), q1[None], [4]))
    return out


def family_masks(rng):
    q = rand_desc(rng)[0]
    out = [case("has_point1 skips", keys([100.0, 120.0], [100.0, 100.0]), np.stack([q, q]), [2, 2],
                keys([300.0], [100.0]), q[None], [2], h1=[1, 0])]
    out.append(_one_query("has_point2 skips the best", [10, 20], [0, 0], rng, h2=[1, 0]))
    return out


def family_epipole(rng):
    out = []
    for o in (0, 3):
        lim = f32(f32(100) * SF[o])
        dx_eq = _float_search(np.sqrt(float(lim)) + 1e-3, lambda v: f32(v * v) == lim)
        for tag, dx in (("below", np.nextafter(dx_eq, f32(0), dtype=np.float32)), ("equal", dx_eq), ("above", f32(dx_eq + f32(0.25)))):
            # the candidate at (0, 100) and the epipole at (dx, 100): distex = dx, distey = 0
            out.append(_one_query("epipole distance^2 %s 100*scale, octave %d" % (tag, o), [25], [0], rng, octave=o, ep=(dx, 100.0), x0=0.0))
    out.append(_one_query("infinite epipole", [25], [0], rng, ep=(np.inf, 100.0)))
    out.append(_one_query("NaN epipole", [25], [0], rng, ep=(np.nan, np.nan)))
    return out


def family_line(rng):
    out = []
    # dsqr = y2^2 for the line y = 0 of KF1 keypoint (100, 0): 3.84f*sigma2 <= dsqr < 3.84*sigma2 (double) at octaves 0, 5, 7
    for o in (0, 5, 7):
        lim_d, lim_f = 3.84 * float(S2[o]), f32(f32(3.84) * S2[o])
        y2 = _float_search(np.sqrt(lim_d), lambda v: float(f32(v * v)) < lim_d and not f32(v * v) < lim_f)
        q = rand_desc(rng)[0]
        out.append(case("dsqr between 3.84f*s2 and 3.84*s2, octave %d" % o, keys([100.0], [0.0]), q[None], [1],
                        keys([250.0], [y2], octave=o), descs(q, [5], rng), [1]))
    q = rand_desc(rng)[0]
    F_D = np.array([[1, 0, 0], [0, 1, 0], [-100, -100, 0]], np.float32)         # a = x1 - 100, b = y1 - 100
    out.append(case("den == 0", keys([100.0], [100.0]), q[None], [1], keys([250.0], [100.0]), q[None], [1], F=F_D))
    F_N = np.array([[-1, -1, 0], [-1, -1, 0], [-0.0, -0.0, 1]], np.float32)     # a = b = -0 at (0, 0)
    out.append(case("den == 0 from -0 coefficients", keys([0.0], [0.0]), q[None], [1], keys([250.0], [100.0]), q[None], [1], F=F_N))
    F_S = np.array([[0, 0, 0], [0, 0, 0], [1e-20, 0, 0]], np.float32)           # a = 1e-20, b = c = 0 at (0, 0): den subnormal
    out.append(case("subnormal den, num == 0", keys([0.0], [0.0]), q[None], [1], keys([0.0], [100.0]), q[None], [1], F=F_S))
    out.append(case("subnormal den, subnormal num^2", keys([0.0], [0.0]), q[None], [1], keys([1.0], [100.0]), q[None], [1], F=F_S))
    return out


def _rot_pairs(name, angles1, angles2, rng, ori=True):
    """KF1 keypoint i matches KF2 keypoint i exactly (own node, own line y = 10 i); angles decide the rotation bins."""
    n = len(angles1)
    d = rand_desc(rng, n)
    k1 = keys([100.0] * n, [10.0 * i for i in range(n)], angle=np.asarray(angles1, np.float32))
    k2 = keys([300.0] * n, [10.0 * i for i in range(n)], angle=np.asarray(angles2, np.float32))
    return case(name, k1, d, list(range(n)), k2, d, list(range(n)), ori=ori)


def family_rotation(rng):
    return [_rot_pairs("rotation wraps below 0", [10.0, 20.0], [350.0, 330.0], rng),
            _rot_pairs("rotation bin 30 -> 0", [895.0, 0.0, 5.0], [0.0, 0.0, 0.0], rng),
            _rot_pairs("0.1 rule: 10 and 1 kept", [0.0] * 10 + [90.0], [0.0] * 11, rng),
            _rot_pairs("0.1 rule: 11 and 1 dropped", [0.0] * 11 + [90.0], [0.0] * 12, rng),
            _rot_pairs("orientation off", [0.0] * 11 + [90.0], [0.0] * 12, rng, ori=False)]


def family_nodes(rng):
    q = rand_desc(rng)[0]
    out = [case("no common node", keys([100.0], [100.0]), q[None], [1], keys([300.0], [100.0]), q[None], [2]),
           case("node on one side only", keys([100.0, 110.0], [100.0, 120.0]), np.stack([q, q]), [1, 2],
                keys([300.0, 310.0], [100.0, 120.0]), np.stack([q, q]), [2, 5])]
    # more than 256 KF2 keypoints in one node (the kernel's path outside the registers)
    n2 = 300
    q1, q2 = rand_desc(rng, 2)
    d2 = rand_desc(rng, n2)
    d2[10], d2[280] = descs(q1, [7, 7], rng)
    d2[100], d2[290] = descs(q2, [9, 9], rng)
    ys = np.full(n2, 100.0)
    ys[290] = 104.0                                                     # q2's later tie fails the line: position 100 wins
    k2 = keys([1.0 + 2.0 * k for k in range(n2)], ys)
    out.append(case("node with 300 KF2 keypoints", keys([50.0, 60.0, 70.0], [100.0, 100.0, 100.0]), np.stack([q1, q2, rand_desc(rng)[0]]),
                    [6, 6, 6], k2, d2, [6] * n2))
    e = np.zeros(0, KEYPOINT_DTYPE)
    out.append(case("n1 = 0", e, np.zeros((0, 32), np.uint8), [], keys([300.0], [100.0]), q[None], [1]))
    out.append(case("n2 = 0", keys([100.0], [100.0]), q[None], [1], e, np.zeros((0, 32), np.uint8), []))
    return out


FAMILIES = {"threshold": family_threshold, "ties": family_ties, "masks": family_masks, "epipole": family_epipole,
            "line": family_line, "rotation": family_rotation, "nodes": family_nodes}
# the edges each family must reach (reference hit counters)
TARGETS = {
    "threshold": ["dist_50", "dist_51", "kept_at_threshold"],
    "ties": ["tie_candidate", "tie_later_wins", "closer_candidate_failed", "line_rejected", "epipole_rejected", "kf2_shared"],
    "masks": ["kf1_has_point", "kf2_has_point"],
    "epipole": ["epipole_rejected", "epipole_equal", "epipole_nonfinite"],
    "line": ["line_float_double_differ", "den_zero", "den_zero_negative_coefficient", "den_subnormal"],
    "rotation": ["rot_negative", "rot_bin_30", "hist_tenth_equal", "hist_dropped"],
    "nodes": ["no_common_node", "node_over_256", "tie_candidate"],
}


def all_cases(seed=0):
    out = []
    for i, (fam, fn) in enumerate(FAMILIES.items()):
        for c in fn(np.random.RandomState(seed * 100 + i)):
            c["family"] = fam
            out.append(c)
    return out


def run_reference(c, rules=T.REFERENCE, hits=None):
    return T.search_for_triangulation(c["k1"], c["d1"], c["h1"], c["fv1"], c["k2"], c["d2"], c["h2"], c["fv2"], c["F"], c["ep"],
                                      SF, S2, c["ori"], rules, hits)


def same(x, y):
    return int(x[0]) == int(y[0]) and np.asarray(x[1]).shape == np.asarray(y[1]).shape and \
        np.asarray(x[1], np.int32).tobytes() == np.asarray(y[1], np.int32).tobytes()


# ---------------------------------------------------------------- GPU
class KeyFrameArrays:
    """What ORBmatcher.SearchForTriangulation reads from a key frame: ext, N, mvKeysUndistorted, mDescriptors."""

    def __init__(self, ext, k, d):
        self.ext = ext
        self.mvKeys = self.mvKeysUndistorted = np.ascontiguousarray(k, KEYPOINT_DTYPE)
        self.mDescriptors = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
        self.N = len(k)


def run_gpu(c, ext):
    import pilotguru_amd as pg
    KF1, KF2 = KeyFrameArrays(ext, c["k1"], c["d1"]), KeyFrameArrays(ext, c["k2"], c["d2"])
    return pg.ORBmatcher(0.6, c["ori"]).SearchForTriangulation(KF1, KF2, c["F"], c["ep"], c["fv1"], c["fv2"], c["h1"], c["h2"])


def run_gpu_batched(cases, ext, extra=5):
    """Every case in ONE pgorb_search_for_triangulation_batch_device launch (one orientation setting): KF1 of case j is frame
    2j, KF2 frame 2j + 1, cap = largest n + extra with NaN keypoints and 0xFF descriptors past n; masks and outputs are
    [npairs][cap] with the padding of the masks set."""
    import torch
    L, h = ext._L, ext._h
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    ori = cases[0]["ori"]
    assert all(c["ori"] == ori for c in cases)
    frames = []
    for c in cases:
        frames += [(c["k1"], c["d1"], c["fv1"]), (c["k2"], c["d2"], c["fv2"])]
    B, P = len(frames), len(cases)
    cap = max(len(k) for k, _, _ in frames) + extra
    kp = np.zeros((B, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["angle"] = np.nan, np.nan, np.nan
    ds = np.full((B, cap, 32), 0xFF, np.uint8)
    fvn = np.full((B, cap), 0xFFFFFFFF, np.uint32); fvs = np.zeros((B, cap + 1), np.int32); fvf = np.full((B, cap), 0xFFFFFFFF, np.uint32)
    n = np.zeros(B, np.int32); nfv = np.zeros(B, np.int32)
    for f, (k, d, fv) in enumerate(frames):
        n[f] = len(k); kp[f, :len(k)] = k; ds[f, :len(k)] = d
        nfv[f] = len(fv[0]); fvn[f, :len(fv[0])] = fv[0]; fvs[f, :len(fv[1])] = fv[1]; fvf[f, :len(fv[2])] = fv[2]
    h1 = np.ones((P, cap), np.uint8); h2 = np.ones((P, cap), np.uint8)
    for j, c in enumerate(cases):
        h1[j, :len(c["h1"])] = c["h1"]; h2[j, :len(c["h2"])] = c["h2"]
    F = np.stack([c["F"].reshape(9) for c in cases]).astype(np.float32)
    ep = np.array([c["ep"] for c in cases], np.float32)
    Tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dk = Tt(kp.view(np.uint8).reshape(B, cap, 28))
    pair1 = torch.arange(0, B, 2, dtype=torch.int32, device="cuda"); pair2 = pair1 + 1
    m12 = torch.full((P, cap), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext._check(L.pgorb_search_for_triangulation_batch_device(h, p(dk), p(Tt(ds)), p(Tt(n)), cap, p(Tt(fvn)), p(Tt(fvs)), p(Tt(fvf)), p(Tt(nfv)),
                                                            p(pair1), p(pair2), P, p(Tt(F)), p(Tt(ep)), p(Tt(h1)), p(Tt(h2)), int(ori), p(m12), p(nm), s))
    torch.cuda.synchronize()
    mh = m12.cpu().numpy()
    assert (mh[:, :] >= -1).all()
    return [(int(nm[j]), mh[j, :len(c["k1"])].copy()) for j, c in enumerate(cases)], mh, n[0::2]


# ---------------------------------------------------------------- synthetic rides: F12 and the epipole from a relative pose
def relative_pose_geometry(t2w, w, h, focal=500.0):
    """F12 and the epipole of key frame 1 at the world origin and key frame 2 at R2w = I, t2w (float32), both with
    K = [[f, 0, w/2], [0, f, h/2], [0, 0, 1]]: LocalMapping::ComputeF12 (src/LocalMapping.cc:538-555) and the epipole of
    ORBmatcher.cc:665-672, in float32 matrix arithmetic."""
    K = np.array([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]], np.float32)
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    R1w, t1w = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R2w, t2w = np.eye(3, dtype=np.float32), np.asarray(t2w, np.float32)
    R12 = R1w @ R2w.T
    t12 = -(R1w @ R2w.T) @ t2w + t1w
    t12x = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], np.float32)
    F12 = (Kinv.T @ t12x @ R12 @ Kinv).astype(np.float32)
    C2 = R2w @ (-R1w.T @ t1w) + t2w                     # pKF1->GetCameraCenter() seen from key frame 2
    with np.errstate(all="ignore"):
        invz = f32(1.0) / f32(C2[2])
        ex = f32(f32(f32(K[0, 0] * C2[0]) * invz) + K[0, 2])
        ey = f32(f32(f32(K[1, 1] * C2[1]) * invz) + K[1, 2])
    return F12, (ex, ey)


def sideways_pose(frames_apart, shift, w, h, focal=500.0):
    """A mostly sideways motion along the ride's image shift: the epipole lies far outside the image and the epipolar lines
    run along the shift, so true matches pass the line test."""
    sx, sy = shift
    return relative_pose_geometry((0.01 * sx * frames_apart, 0.01 * sy * frames_apart, 1e-4), w, h, focal)


def forward_pose(epipole, w, h, focal=500.0):
    """A forward motion whose epipole lands at `epipole` (inside the image)."""
    ex, ey = epipole
    return relative_pose_geometry(((ex - w / 2.0) / focal, (ey - h / 2.0) / focal, 1.0), w, h, focal)
