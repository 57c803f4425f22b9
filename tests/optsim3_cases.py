"""Constructed loop candidates for pgorb_optimize_sim3 (pilotguru_amd/csrc/optimize_sim3.hip) and the runners that put them through
the plain reference (tests/optsim3_reference.py), the single call and the batched device form.  A helper module (no tests):
tests/test_optimize_sim3.py and tests/golden/make_optsim3_spread.py use it.

A scene is two key frames with poses and cameras of their own and a true Sim3 S12 between their camera frames.  KF2's points are
seen at 2-8 m inside its 640 x 480 image; KF1's points are X1c = s*R*X2c + t; each goes to the world through its key frame's
pose, and each key frame's keypoint is the projection of its own point (plus level-scaled pixel noise and gross outliers where
asked for).  The start is the true Sim3 moved by a left update.  Seeds are fixed; the CPU tests hold every case to the case
condition (`condition`) -- a case that breaks it is rebuilt with another seed, never skipped."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optsim3_reference as OR  # noqa: E402
from sim3_cases import make_pose, rotation  # noqa: E402

f32, f64 = np.float32, np.float64
NLEVELS = 8
K1 = (500.0, 500.0, 320.0, 240.0)
K2_OTHER = (430.0, 445.0, 300.0, 255.0)
INV_SIGMA2 = OR.inv_level_sigma2(1.2, NLEVELS)
SF = np.array([1.2 ** i for i in range(NLEVELS)])
MAX_N = 16000
TH2 = 10.0
SPREAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optsim3_spread.json")
EXACT = OR.LibM(False)


class Case:
    def __init__(self, name, keys1, octaves1, pose1, kf_point1, keys2, octaves2, pose2, kf_point2, matches12, new_matches12, points, bad,
                 estimate, fix_scale=0, th2=TH2, true=None):
        self.name = name
        self.keys1, self.keys2 = np.asarray(keys1, f32).reshape(-1, 2), np.asarray(keys2, f32).reshape(-1, 2)
        self.octaves1, self.octaves2 = np.asarray(octaves1, np.int32), np.asarray(octaves2, np.int32)
        self.pose1, self.pose2 = pose1, pose2
        self.kf_point1, self.kf_point2 = np.asarray(kf_point1, np.int32), np.asarray(kf_point2, np.int32)
        self.matches12 = np.asarray(matches12, np.int32)
        self.new_matches12 = None if new_matches12 is None else np.asarray(new_matches12, np.int32)
        self.points = np.asarray(points, f32).reshape(-1, 3)
        self.bad = None if bad is None else np.asarray(bad, np.uint8)
        self.estimate = (np.asarray(estimate[0], f32).reshape(9), np.asarray(estimate[1], f32).reshape(3), f32(estimate[2]))
        self.fix_scale, self.th2, self.true = int(fix_scale), float(th2), true

    @property
    def n1(self):
        return len(self.matches12)

    @property
    def n2(self):
        return len(self.kf_point2)


def project(X, cam):
    return np.stack([X[:, 0] / X[:, 2] * cam[0] + cam[2], X[:, 1] / X[:, 2] * cam[1] + cam[3]], 1)


def scene(name, seed, m, n_out=0, s=1.0, rot=0.2, noise=0.0, start=(0.02, 0.05, 0.03), fix_scale=0, cam2=K1, octaves="zero", sparse=0,
          new_matches=0, identity=False):
    """m correspondences of which n_out have a grossly wrong KF1 observation.  start = the sizes of the left update (omega, upsilon,
    sigma) that moves the true Sim3 to the input estimate (None: start at the truth).  sparse: that many further KF1 keypoints that
    drop out (an empty KF1 slot, a KF2 keypoint without a slot, a bad point, no match, in turn).  new_matches: that many
    correspondences whose matches12 entry is -1 or wrong and whose true match arrives in new_matches12."""
    rng = np.random.RandomState(seed)
    Rs, ts = (np.eye(3), np.zeros(3)) if identity else (rotation(rng.uniform(-1, 1, 3) * rot), rng.uniform(-0.3, 0.3, 3))
    u, v, z = rng.uniform(60, 580, m), rng.uniform(60, 420, m), rng.uniform(2.0, 8.0, m)
    if identity:                                                        # projections that are exact in binary: the errors at the truth are 0
        u, v, z = 320.0 + 125.0 * rng.randint(-2, 3, m), 240.0 + 125.0 * rng.randint(-1, 2, m), 2.0 ** rng.randint(1, 4, m)
    X2c = np.stack([(u - cam2[2]) * z / cam2[0], (v - cam2[3]) * z / cam2[1], z], 1)
    X1c = s * X2c @ Rs.T + ts
    if identity:
        R1 = R2 = np.eye(3)
        t1 = t2 = np.zeros(3)
    else:
        R1, t1 = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-2, 2, 3)
        R2, t2 = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-2, 2, 3)
    P1w, P2w = (X1c - t1) @ R1, (X2c - t2) @ R2
    o1 = np.zeros(m, np.int32) if octaves == "zero" else rng.randint(0, NLEVELS, m).astype(np.int32)
    o2 = np.zeros(m, np.int32) if octaves == "zero" else rng.randint(0, NLEVELS, m).astype(np.int32)
    uv1, uv2 = project(X1c, K1), project(X2c, cam2)
    if noise:
        uv1 = uv1 + rng.normal(0, noise, uv1.shape) * SF[o1][:, None]
        uv2 = uv2 + rng.normal(0, noise, uv2.shape) * SF[o2][:, None]
    outl = rng.permutation(m)[:n_out]
    uv1[outl] += rng.uniform(25, 80, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2)) * SF[o1[outl]][:, None]
    # the key frames: KF1's keypoints in order with `sparse` drop-outs spread between them; KF2's keypoints permuted, three spare
    n1, n2 = m + sparse, m + 3
    slot_of = np.sort(rng.permutation(n1)[:m])
    perm2 = rng.permutation(n2)[:m]
    empty2 = np.setdiff1d(np.arange(n2), perm2)
    points = list(P2w) + list(P1w)
    kf1, kf2, m12 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32), np.full(n1, -1, np.int32)
    keys1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1)
    keys2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
    oct1, oct2 = rng.randint(0, NLEVELS, n1).astype(np.int32), rng.randint(0, NLEVELS, n2).astype(np.int32)
    kf2[perm2], oct2[perm2], keys2[perm2] = np.arange(m), o2, uv2
    kf1[slot_of], m12[slot_of], oct1[slot_of], keys1[slot_of] = m + np.arange(m), perm2, o1, uv1
    bad = np.zeros(2 * m + sparse, np.uint8)
    for j, i in enumerate(np.setdiff1d(np.arange(n1), slot_of)):
        kind = j % 4
        if kind == 0:                                                   # matched, but KF1's slot is empty
            m12[i] = perm2[j % m]
        elif kind == 1:                                                 # matched to a KF2 keypoint without a point
            kf1[i], m12[i] = m + (j % m), empty2[j % 3]
        elif kind == 2:                                                 # a consistent pair whose KF1 point is bad
            points.append(P1w[j % m])
            kf1[i], m12[i], keys1[i], oct1[i] = len(points) - 1, perm2[j % m], uv1[j % m], o1[j % m]
            bad[kf1[i]] = 1
        else:                                                           # a point, no match
            kf1[i] = m + (j % m)
    nm = None
    if new_matches:
        nm = np.full(n1, -1, np.int32)
        for k, i in enumerate(slot_of[rng.permutation(m)[:new_matches]]):
            nm[i] = m12[i]
            m12[i] = -1 if k % 2 == 0 else perm2[(int(np.nonzero(perm2 == m12[i])[0][0]) + 1) % m]      # absent, or another point's keypoint
    true = OR.Sim3(OR.quat_from_matrix(Rs), ts, s)
    st = true
    if start is not None:
        upd = np.concatenate([rng.normal(0, 1, 3) * start[0], rng.normal(0, 1, 3) * start[1], [0.0 if fix_scale else rng.choice([-1, 1]) * start[2]]])
        st = OR.sim3_mul(OR.sim3_exp(upd, EXACT), true)
    est = (OR.matrix_from_quat(st.q / np.linalg.norm(st.q)), st.t, st.s)
    return Case(name, keys1, oct1, make_pose(R1, t1, K1), kf1, keys2, oct2, make_pose(R2, t2, cam2), kf2, m12, nm, np.array(points, f64).astype(f32),
                bad[:len(points)] if sparse else None, est, fix_scale, true=(Rs, ts, s))


def _cases():
    return [
        scene("clean_10", 1, 10), scene("noisy_11", 102, 11, noise=0.4), scene("noisy_63", 203, 63, noise=0.5, octaves="mixed"),
        scene("noisy_64", 2065, 64, 3, noise=0.5, octaves="mixed", fix_scale=1), scene("noisy_65", 5, 65, 4, noise=0.5, cam2=K2_OTHER),
        scene("noisy_256", 106, 256, noise=0.7, octaves="mixed", s=1.7), scene("outliers_257", 1007, 257, 30, noise=0.7, octaves="mixed", s=0.6, sparse=40),
        scene("outliers_300", 8, 300, 45, noise=0.8, octaves="mixed", cam2=K2_OTHER, sparse=60, new_matches=20, rot=0.6, start=(0.1, 0.2, 0.1)),
        scene("dropped_40", 109, 40, 2, noise=0.5, sparse=24, octaves="mixed"),
        scene("ten_left", 110, 13, 3, noise=0.3), scene("nine_left", 11, 12, 3, noise=0.3), scene("few_0", 12, 0), scene("few_9", 113, 9),
        scene("start_at_truth", 14, 30, start=None, identity=True), scene("start_at_truth_fixed", 15, 30, start=None, identity=True, fix_scale=1),
        scene("far_start", 116, 80, 8, noise=0.5, start=(0.25, 0.8, 0.4), octaves="mixed"),
        scene("far_start_fixed", 1064, 80, 8, noise=0.5, start=(0.25, 0.8, 0.0), fix_scale=1, octaves="mixed"),
        scene("new_matches_50", 18, 50, 5, noise=0.5, new_matches=12, octaves="mixed", sparse=9),
        # so far off and so noisy that the first call does not converge: edges leave the kernel's quadratic zone again in the second
        scene("huber_second_call", 3004, 60, 12, noise=1.2, start=(0.4, 1.2, 0.4), octaves="mixed"),
    ]


CASE_NAMES = ["clean_10", "noisy_11", "noisy_63", "noisy_64", "noisy_65", "noisy_256", "outliers_257", "outliers_300", "dropped_40", "ten_left",
              "nine_left", "few_0", "few_9", "start_at_truth", "start_at_truth_fixed", "far_start", "far_start_fixed", "new_matches_50", "huber_second_call"]
_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
        assert [c.name for c in _CASES] == CASE_NAMES
    return _CASES


def case(name):
    return all_cases()[CASE_NAMES.index(name)]


def run_reference(c, form="edges", rules=OR.REFERENCE, hits=None, trace=None):
    return OR.optimize_sim3(c.keys1, c.octaves1, c.pose1, c.kf_point1, c.keys2, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.new_matches12,
                            c.points, c.bad, c.estimate, c.th2, c.fix_scale, INV_SIGMA2, form, rules, hits, trace)


_REF = {}


def reference(c):
    """The reference's result, trace and hits under every form, computed once and shared; treat as read-only."""
    if c.name not in _REF:
        r = {}
        for form in OR.FORMS:
            hits, trace = {}, {}
            r[form] = (run_reference(c, form, hits=hits, trace=trace), trace, hits)
        _REF[c.name] = r
    return _REF[c.name]


# ---------------------------------------------------------------- tolerances (tests/golden/optsim3_spread.json)
FLOAT_OUTPUTS = ("R", "t", "s", "scw_R", "scw_t", "scw_Ow", "chi2")
INT_FIELDS = ("ret", "status", "ncorr", "nbad", "iterations", "trials", "more", "matches12_out")


def scaled_differences(a, b):
    """The largest difference per float output between two results, scaled by 1 for rotation entries, by max(1, |.|inf) for the
    translations, the scale and Ow, and by max(1, chi2) for both chi2 vectors."""
    rel = lambda x, y: float(np.abs(np.asarray(x, f64) - np.asarray(y, f64)).max()) / max(1.0, float(np.abs(np.asarray(x, f64)).max()))
    d = dict(R=float(np.abs(np.asarray(a["R"], f64) - np.asarray(b["R"], f64)).max()), t=rel(a["t"], b["t"]), s=rel([a["s"]], [b["s"]]),
             scw_R=0.0, scw_t=0.0, scw_Ow=0.0, chi2=0.0)
    if a["scw_Tcw"] is not None and b["scw_Tcw"] is not None:
        Ta, Tb = np.asarray(a["scw_Tcw"], f64).reshape(3, 4), np.asarray(b["scw_Tcw"], f64).reshape(3, 4)
        d.update(scw_R=float(np.abs(Ta[:, :3] - Tb[:, :3]).max()), scw_t=rel(Ta[:, 3], Tb[:, 3]), scw_Ow=rel(a["scw_Ow"], b["scw_Ow"]))
    for k in ("chi2_12", "chi2_21"):
        ca, cb = np.asarray(a[k], f64), np.asarray(b[k], f64)
        if len(ca):
            d["chi2"] = max(d["chi2"], float((np.abs(ca - cb) / np.maximum(1.0, np.abs(ca))).max()))
    return d


def spread(c):
    """The largest scaled difference per output between any two of the reference's forms."""
    rs = [reference(c)[form][0] for form in OR.FORMS]
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for i in range(len(rs)):
        for j in range(i + 1, len(rs)):
            d = scaled_differences(rs[i], rs[j])
            out = {k: max(out[k], d[k]) for k in out}
    return out


def recorded_spread():
    with open(SPREAD_FILE) as f:
        return json.load(f)["spread"]


ULP1 = float(np.spacing(f32(1.0)))


def bounds(recorded):
    """pose_cases.bounds' rule: the larger of 2 float ulps at the output's scale (the differences are scaled to 1) and 16 x the
    spread the reference shows between its forms."""
    return {k: max(2.0 * ULP1, 16.0 * float(recorded[k])) for k in FLOAT_OUTPUTS}


def differences(c, want, got, recorded):
    """The compared outputs that differ: integers exactly, the estimate of an untouched problem as bytes, floats by bounds()."""
    bad = [k for k in INT_FIELDS if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    if want["status"]:
        for k in ("R", "t", "s"):
            if np.asarray(want[k], f32).tobytes() != np.asarray(got[k], f32).tobytes():
                bad.append(k + " bytes")
        if want["status"] & OR.OS3_NONFINITE and (np.asarray(got["chi2_12"]).any() or np.asarray(got["chi2_21"]).any()):
            bad.append("chi2")
    if want["status"] & OR.OS3_NONFINITE:
        return bad
    d, b = scaled_differences(want, got), bounds(recorded)
    return bad + ["%s %.3g > %.3g" % (k, d[k], b[k]) for k in FLOAT_OUTPUTS if not d[k] <= b[k]]


def condition(c):
    """The case condition: across all forms the Levenberg trace (iterations, trials, accept or reject per trial, of both calls) and
    every classification are identical, and no chi2 at either classification lies within 1e-4 relative of th2.  Returns the list
    of violations."""
    ref = reference(c)
    r0, t0, _ = ref[OR.FORMS[0]]
    why = []
    th2 = float(f32(c.th2))
    for form in OR.FORMS:
        r, t, _ = ref[form]
        if t["lm"] != t0["lm"] or r["iterations"] != r0["iterations"] or r["trials"] != r0["trials"]:
            why.append("%s: the Levenberg trace differs under %s" % (c.name, form))
        if len(t["cls"]) != len(t0["cls"]) or any(not np.array_equal(a[0], b[0]) for a, b in zip(t["cls"], t0["cls"])):
            why.append("%s: a classification differs under %s" % (c.name, form))
        for over, c12, c21, act in t["cls"]:
            for v in (c12[act], c21[act]):
                if len(v) and float(np.abs(v - th2).min()) <= 1e-4 * th2:
                    why.append("%s: a chi2 within 1e-4 of th2 under %s" % (c.name, form))
    return why


# ---------------------------------------------------------------- GPU runners
def table(points):
    from pilotguru_amd.orb import MAP_POINT_DTYPE
    pts = np.zeros(max(len(points), 1), MAP_POINT_DTYPE)
    pts["pos"][:len(points)] = points
    return pts


def keypoints(xy, octaves):
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(len(octaves), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], octaves
    return k


def pose_record(pose):
    from pilotguru_amd.orb import kf_pose
    return kf_pose(np.asarray(pose["Tcw"], f32).reshape(3, 4), np.zeros(3, f32), pose["fx"], pose["fy"], pose["cx"], pose["cy"])


def estimate_record(est):
    from pilotguru_amd.orb import SIM3_ESTIMATE_DTYPE
    e = np.zeros(1, SIM3_ESTIMATE_DTYPE)
    e["R12"], e["t12"], e["s12"] = est[0], est[1], est[2]
    return e


def result_of(ret, est_out, mout, c12, c21, scw, info, status_known=True):
    st = int(info[0])
    return dict(ret=int(ret), R=np.array(est_out["R12"], f32).reshape(9), t=np.array(est_out["t12"], f32).reshape(3), s=f32(est_out["s12"]),
                matches12_out=np.asarray(mout, np.int32), chi2_12=np.asarray(c12, f32), chi2_21=np.asarray(c21, f32),
                scw_Tcw=None if st else np.array(scw["Tcw"], f32).reshape(12), scw_Ow=None if st else np.array(scw["Ow"], f32).reshape(3),
                status=st, ncorr=int(info[1]), nbad=int(info[2]), iterations=[int(info[3]), int(info[5])], trials=[int(info[4]), int(info[6])],
                more=int(info[7]), scw=np.array(scw).copy(), bytes=np.asarray(est_out).tobytes() + np.asarray(scw).tobytes())


def run_gpu(c, ext):
    """The single call through the C ABI."""
    from pilotguru_amd.orb import KF_POSE_DTYPE, SIM3_ESTIMATE_DTYPE
    L, h = ext._L, ext._h
    k1, k2, pts = keypoints(c.keys1, c.octaves1), keypoints(c.keys2, c.octaves2), table(c.points)
    P1, P2 = np.asarray(pose_record(c.pose1)).reshape(1), np.asarray(pose_record(c.pose2)).reshape(1)
    n1 = c.n1
    eo, sp = np.zeros(1, SIM3_ESTIMATE_DTYPE), np.zeros(1, KF_POSE_DTYPE)
    mo, c12, c21, info = np.full(max(n1, 1), -9, np.int32), np.full(max(n1, 1), -9, f32), np.full(max(n1, 1), -9, f32), np.full(8, -9, np.int32)
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(x) for x in (c.kf_point1, c.kf_point2, c.matches12)]
    nm = None if c.new_matches12 is None else np.ascontiguousarray(c.new_matches12)
    bad = None if c.bad is None else np.ascontiguousarray(c.bad)
    ret = L.pgorb_optimize_sim3(h, p(k1), n1, p(P1), p(keep[0]), p(k2), c.n2, p(P2), p(keep[1]), p(keep[2]), p(nm), len(c.points), p(pts), p(bad),
                                p(estimate_record(c.estimate)), C.c_float(c.th2), c.fix_scale, p(eo), p(mo), p(c12), p(c21), p(sp), p(info))
    if ret < 0:
        return ret
    return result_of(ret, eo[0], mo[:n1], c12[:n1], c21[:n1], sp[0], info)


def run_gpu_batch(cases, ext, order=None, stream=None):
    """One launch of pgorb_optimize_sim3_batch_device per (th2, fix_scale) group over the cases in `order`: every case brings two
    frames of its own and a slice of one shared table.  Returns the per-case results in that order."""
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, SIM3_ESTIMATE_DTYPE, MAP_POINT_DTYPE
    L, h = ext._L, ext._h
    order = list(range(len(cases))) if order is None else list(order)
    cs = [cases[j] for j in order]
    res = [None] * len(cs)
    st = torch.cuda.current_stream() if stream is None else stream
    for key in sorted({(c.th2, c.fix_scale) for c in cs}):
        idx = [j for j, c in enumerate(cs) if (c.th2, c.fix_scale) == key]
        grp = [cs[j] for j in idx]
        cap = max(max(c.n1, c.n2, 1) for c in grp) + 3                  # not a multiple of 64 in general; the rows' tails are garbage
        nf, npair = 2 * len(grp), len(grp)
        kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["octave"] = np.nan, np.nan, 99             # past n: never read
        slots = np.full((nf, cap), 12345678, np.int32)
        m12, nm12 = np.full((npair, cap), 12345678, np.int32), np.full((npair, cap), -1, np.int32)
        poses, ests = np.zeros(nf, KF_POSE_DTYPE), np.zeros(npair, SIM3_ESTIMATE_DTYPE)
        ns = np.zeros(nf, np.int32)
        off, tabs, bads = 0, [], []
        for j, c in enumerate(grp):
            kp[2 * j, :c.n1], kp[2 * j + 1, :c.n2] = keypoints(c.keys1, c.octaves1), keypoints(c.keys2, c.octaves2)
            slots[2 * j, :c.n1] = np.where(c.kf_point1 >= 0, c.kf_point1 + off, -1)
            slots[2 * j + 1, :c.n2] = np.where(c.kf_point2 >= 0, c.kf_point2 + off, -1)
            m12[j, :c.n1] = c.matches12
            if c.new_matches12 is not None:
                nm12[j, :c.n1] = c.new_matches12
            poses[2 * j], poses[2 * j + 1] = pose_record(c.pose1), pose_record(c.pose2)
            ests[j] = estimate_record(c.estimate)[0]
            ns[2 * j], ns[2 * j + 1] = c.n1, c.n2
            tabs.append(c.points)
            bads.append(np.zeros(len(c.points), np.uint8) if c.bad is None else c.bad)
            off += len(c.points)
        pts = table(np.concatenate(tabs) if off else np.zeros((0, 3), f32))
        bad = np.concatenate(bads + [np.zeros(1, np.uint8)])
        keep = []

        def p(t):
            keep.append(t)
            return C.c_void_p(t.data_ptr())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        with torch.cuda.stream(st):
            full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device="cuda")
            o_e, o_sp = full((npair, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8), full((npair, KF_POSE_DTYPE.itemsize), torch.uint8)
            o_m, o_c1, o_c2 = full((npair, cap), torch.int32), full((npair, cap), torch.float32), full((npair, cap), torch.float32)
            o_info, o_n = full((npair, 8), torch.int32), full((npair,), torch.int32)
            ext._check(L.pgorb_optimize_sim3_batch_device(
                h, p(dev(kp.view(np.uint8).reshape(nf, cap, KEYPOINT_DTYPE.itemsize))), p(dev(ns)), cap,
                p(dev(np.arange(0, nf, 2, dtype=np.int32))), p(dev(np.arange(1, nf, 2, dtype=np.int32))), npair,
                p(dev(poses.view(np.uint8).reshape(nf, -1))), p(dev(slots)), p(dev(m12)), p(dev(nm12)), off,
                p(dev(pts.view(np.uint8).reshape(len(pts), MAP_POINT_DTYPE.itemsize))), p(dev(bad)),
                p(dev(ests.view(np.uint8).reshape(npair, -1))), C.c_float(key[0]), key[1], p(o_e), p(o_m), p(o_c1), p(o_c2), p(o_sp), p(o_info),
                p(o_n), C.c_void_p(st.cuda_stream)))
        st.synchronize()
        eo = np.frombuffer(o_e.cpu().numpy().tobytes(), SIM3_ESTIMATE_DTYPE)
        sp = np.frombuffer(o_sp.cpu().numpy().tobytes(), KF_POSE_DTYPE)
        mo, c1, c2, info, nin = (t.cpu().numpy() for t in (o_m, o_c1, o_c2, o_info, o_n))
        for j, c in enumerate(grp):
            r = result_of(nin[j], eo[j], mo[j, :c.n1], c1[j, :c.n1], c2[j, :c.n1], sp[j], info[j])
            r["tail_ok"] = bool((mo[j, c.n1:] == -1).all() and (c1[j, c.n1:] == 0).all() and (c2[j, c.n1:] == 0).all())
            res[idx[j]] = r
    return res


# ---------------------------------------------------------------- the chain of ComputeSim3, steps 1-5
CHAIN_SEEDS = (21, 22, 23)
CHAIN_TH = 10                     # SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10)


def chain_case(pc, matches12, new_matches12, estimate, name=None):
    """The OptimizeSim3 problem on the loop pair `pc` (a loop_cases.PairCase) after the solver gave matches12 and the estimate and
    SearchBySim3 gave new_matches12."""
    k1, k2 = pc.kf1[0], pc.kf2[0]
    pose = lambda P: dict(Tcw=np.array(P["Tcw"], f32), fx=f32(P["fx"]), fy=f32(P["fy"]), cx=f32(P["cx"]), cy=f32(P["cy"]))  # noqa: E731
    return Case(name or "optsim3_" + pc.name, np.stack([k1["x"], k1["y"]], 1), k1["octave"], pose(pc.kf1[2]), pc.slots1,
                np.stack([k2["x"], k2["y"]], 1), k2["octave"], pose(pc.kf2[2]), pc.slots2, matches12, new_matches12,
                np.array([p["pos"] for p in pc.points], f32), np.array([bool(p.get("bad", False)) for p in pc.points], np.uint8), estimate)


_CHAIN = {}


def chain_reference(seed):
    """sim3_cases.chain_reference (steps 1-3 through their references) and the OptimizeSim3 case that follows from them."""
    import sim3_cases as SC
    if seed not in _CHAIN:
        ch = SC.chain_reference(seed)
        pc, r, (n3, s12) = ch[0], ch[5], ch[6]
        _CHAIN[seed] = ch + (chain_case(pc, r["matches12_out"], s12, (r["found_R"], r["found_t"], r["found_s"])),)
    return _CHAIN[seed]
