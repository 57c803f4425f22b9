"""Constructed maps for pgorb_global_bundle_adjustment (pilotguru_amd/csrc/global_ba.hip) and the runners that put them through the
plain reference (tests/gba_reference.py), the single call and the device form.  A helper module (no tests);
tests/test_global_bundle_adjustment.py and tests/golden/make_gba_spread.py use it.

The scenes are lba_cases.Builder's: pixel noise keeps the optimum's chi2 macroscopic and a few far points keep every iteration's
improvement far above the rounding of the chi2 sum, so Levenberg's decisions stay away from their thresholds (`condition`)."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gba_reference as GR  # noqa: E402
import lba_cases as LC  # noqa: E402
import lba_reference as LR  # noqa: E402
import pose_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
SPREAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gba_spread.json")
CASE_NAMES = ["init2", "chain5", "ring24", "robust", "bad", "no_gauge", "nothing", "nonfinite", "wide", "envelope_limit"]
ONE_FORM = ("wide", "envelope_limit")      # the reference runs these under one form in the suite; their spread is recorded once
TWIST = (0.004, 0.02)


def _line(B, ncam, span, twist_from=1):
    rng = B.rng
    xs = np.linspace(-span, span, ncam) if ncam > 1 else np.array([0.0])
    return [B.add_camera([xs[c], rng.normal(0, 0.1), rng.normal(0, 0.1)], LC.CAM_A, TWIST if c >= twist_from else None) for c in range(ncam)]


def _point(B, x, far=False):
    rng = B.rng
    X = [x + rng.uniform(-0.6, 0.6), rng.uniform(-1.0, 1.0), rng.uniform(40, 60) if far else rng.uniform(4, 9)]
    return B.add_point(X, 0.5 if far else 0.04)


def _chain(seed, ncam, npts, nobs=3, outliers=0, id0=0, far=3, noise=0.7, name=""):
    """Cameras on a line, point k seen by `nobs` consecutive cameras."""
    B = LC.Builder(seed)
    rng = B.rng
    cams = _line(B, ncam, 0.5 * (ncam - 1) * 0.6, 1 if id0 is not None else 0)
    pending = []
    for k in range(npts):
        c0 = int(rng.integers(0, max(ncam - nobs + 1, 1)))
        p = _point(B, -0.5 * (B.true_T[cams[c0]].t[0] + B.true_T[cams[min(c0 + nobs, ncam) - 1]].t[0]), k < far)     # between its cameras
        pending += [(p, cams[c]) for c in range(c0, min(c0 + nobs, ncam))]
    bad_ones = set(int(i) for i in rng.choice(len(pending), outliers, replace=False)) if outliers else set()
    for i, (p, f) in enumerate(pending):
        off = None
        if i in bad_ones:
            a = rng.uniform(0, 2 * np.pi)
            off = np.array([np.cos(a), np.sin(a)]) * rng.uniform(25, 60)
        B.observe(p, f, noise, offset=off)
    return B, cams


def _problem(B, id0, name):
    return B.problem([], id0, name, extra_keys=2)


def make_case(name):
    """(problem, iterations, robust, in_place)"""
    if name == "init2":
        B, cams = _chain(1102, 2, 60, nobs=2)
        return _problem(B, 0, name), 20, 0, 1
    if name == "chain5":
        B, cams = _chain(1105, 5, 80)
        return _problem(B, 0, name), 10, 0, 0
    if name == "ring24":
        B, cams = _chain(1124, 24, 170)
        for k in range(8):                                      # the closing points: seen by 22, 23, 0 and 1 -- fill in the skyline
            p = B.add_point([B.rng.uniform(-1, 1), B.rng.uniform(-1, 1), B.rng.uniform(25, 35)], 0.3)
            for f in (22, 23, 0, 1):
                B.observe(p, f)
        return _problem(B, 0, name), 10, 0, 0
    if name == "robust":
        B, cams = _chain(1105, 5, 80, outliers=14, noise=1.0)
        return _problem(B, 0, name), 10, 1, 0
    if name == "bad":
        B, cams = _chain(1107, 6, 70)
        rng = B.rng
        badf = [B.add_camera([0.0, -0.5, 0.0], bad=True), B.add_camera([0.4, -0.6, 0.0], bad=True)]
        for q in rng.choice(np.arange(3, 40), 9, replace=False):
            B.observe(int(q), badf[int(q) % 2])
        p = B.add_point([0.9, 0.1, 7.0], bad=True)             # a bad point with observations
        B.observe(p, cams[1])
        B.observe(p, cams[2])
        p = B.add_point([-0.4, 0.3, 6.0])                      # a point whose only observations are in bad key frames
        B.observe(p, badf[0])
        B.observe(p, badf[1])
        B.add_point([0.2, 0.2, 5.0])                           # a point nobody observes
        B.add_camera([0.1, 0.7, 0.0], twist=TWIST)             # a live key frame with no edge
        return _problem(B, 0, name), 10, 0, 1
    if name == "no_gauge":
        B, cams = _chain(1132, 4, 50, id0=None)
        return _problem(B, None, name), 10, 0, 0
    if name == "nothing":
        B, cams = _chain(1141, 3, 12)
        B.pbad = [1] * len(B.pbad)
        return _problem(B, 0, name), 10, 0, 1
    if name == "nonfinite":
        B, cams = _chain(1151, 3, 20)
        c = B.add_camera([0.25, -0.5, 0.125], tilt=0.0)        # identity rotation, dyadic centre: the point below maps to (0, 0, 0)
        p = B.add_point([0.25, -0.5, 0.125], start=[0.25, -0.5, 0.125])
        B.observe(p, c, xy=[100.0, 100.0], octave=0)
        B.observe(p, cams[1], xy=[200.0, 150.0], octave=0)
        return _problem(B, 0, name), 10, 0, 1
    if name == "wide":
        B, cams = _chain(1170, 70, 2900, far=6)
        rng = B.rng
        hub = B.add_point([0.0, 0.0, 30.0], 0.3)              # one point observed by 40 key frames
        for f in range(15, 55):
            B.observe(hub, f)
        for k in range(1100):                                  # one camera with more than 1024 edges
            p = B.add_point([rng.uniform(-1.5, 1.5) - B.true_T[35].t[0], rng.uniform(-1.0, 1.0), rng.uniform(4, 9)], 0.04)
            B.observe(p, 35)
            B.observe(p, 34 + 2 * int(k % 2))
        return B.problem([], 0, name, extra_keys=0), 2, 0, 0
    if name == "envelope_limit":
        B = LC.Builder(1513)
        for c in range(513):
            B.add_camera([0.01 * (c - 256), 0.0, 0.0], LC.CAM_A, TWIST)
        p = B.add_point([0.0, 0.0, 8.0])
        for c in range(513):
            B.observe(p, c, octave=c % LC.NLEVELS)
        return B.problem([], None, name, extra_keys=0), 10, 0, 1      # no gauge: 513 rows, 513 * 514 / 2 = 131841 blocks
    raise KeyError(name)


_cache, _ref_cache = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = make_case(name)
    return _cache[name]


def run_reference(name, rules=GR.REFERENCE, form=GR.Form()):
    key = (name, rules, form)
    if key not in _ref_cache:
        P, its, robust, _ = case(name)
        _ref_cache[key] = GR.global_bundle_adjustment(P, its, robust, rules, form)
    return _ref_cache[key]


# ---------------------------------------------------------------- tolerances (tests/golden/gba_spread.json)
FLOAT_OUTPUTS = ("R", "t", "Ow", "pos", "chi2")
DECISIONS = ("rho", "stop", "pivot")
INT_OUTPUTS = ("ret", "kf_done", "point_done", "info", "pose_is_input")
bounds, window_of, ULP1 = LC.bounds, LC.window_of, LC.ULP1


def scaled_differences(P, a, b):
    """lba_cases.scaled_differences over every key frame and every point: rotation entries as they are, tcw, Ow and pos over
    max(1, |.|inf) of the vector, chi2 over max(1, chi2)."""
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for f in range(P.nframes):
        if P.kf_bad[f]:                                         # the input's bytes: compared as bytes
            continue
        Ta, Tb = a["pose_Tcw"][f].astype(f64).reshape(3, 4), b["pose_Tcw"][f].astype(f64).reshape(3, 4)
        out["R"] = max(out["R"], float(np.abs(Ta[:, :3] - Tb[:, :3]).max()))
        out["t"] = max(out["t"], float(np.abs(Ta[:, 3] - Tb[:, 3]).max()) / max(1.0, float(np.abs(Ta[:, 3]).max())))
        oa, ob = a["pose_Ow"][f].astype(f64), b["pose_Ow"][f].astype(f64)
        out["Ow"] = max(out["Ow"], float(np.abs(oa - ob).max()) / max(1.0, float(np.abs(oa).max())))
    pa, pb = a["pos"].astype(f64), b["pos"].astype(f64)
    if len(pa):
        out["pos"] = float((np.abs(pa - pb).max(1) / np.maximum(1.0, np.abs(pa).max(1))).max())
    ca, cb = a["chi2"].astype(f64), b["chi2"].astype(f64)
    if len(ca):
        out["chi2"] = float((np.abs(ca - cb) / np.maximum(1.0, np.abs(ca))).max())
    return out


def spread(name, forms=None):
    """Per float output the largest scaled difference between any two of the reference's arithmetic forms, and per decision quantity
    the largest difference of its margin between the forms (lba_cases.spread)."""
    P = case(name)[0]
    rs = [run_reference(name, form=fm) for fm in (GR.FORMS if forms is None else forms)]
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for i in range(len(rs)):
        for j in range(i + 1, len(rs)):
            d = scaled_differences(P, rs[i], rs[j])
            out = {k: max(out[k], d[k]) for k in out}
    for k in DECISIONS:
        v = [r["margins"][k] for r in rs if k in r["margins"] and np.isfinite(r["margins"][k])]
        out["decision_" + k] = float(max(v) - min(v)) if v else 0.0
    return out


def recorded():
    with open(SPREAD_FILE) as f:
        return json.load(f)


def recorded_spread():
    return recorded()["spread"]


def condition(name, rec, forms=None):
    """What breaks the case condition under any form: a Levenberg decision (rho's sign, the 1e3 rule, a pivot's sign) nearer its
    threshold than lba_cases.window_of allows, or integer outputs that differ between the forms."""
    base = run_reference(name)
    bad = []
    for fm in (GR.FORMS if forms is None else forms):
        r = run_reference(name, form=fm)
        m = r["margins"]
        for k in DECISIONS:
            w = window_of(rec, k)
            lim = {"stop": 1e3 * w}.get(k, w)
            if k in m and not m[k] > lim:
                bad.append("%s under %s: %s margin %.3g <= %.3g" % (name, fm, k, m[k], lim))
        for k in INT_OUTPUTS:
            if not np.array_equal(r[k], base[k]):
                bad.append("%s under %s: %s differs from the default form" % (name, fm, k))
    return bad


def differences(P, want, got, rec):
    """The compared outputs that differ: integers, flags and statuses exactly; a pose that is the input's bytes as bytes; floats by
    bounds(); with a status pos as bytes and chi2 all 0."""
    bad = [k for k in INT_OUTPUTS if k != "pose_is_input" and not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    for f in np.flatnonzero(want["pose_is_input"]):
        if got["pose_bytes"][f] != got["pose_in_bytes"][f]:
            bad.append("pose bytes of key frame %d" % f)
    if not got["camera_kept"]:
        bad.append("camera")
    if want["info"][0]:
        if want["pos"].tobytes() != got["pos"].tobytes():
            bad.append("pos bytes")
        if got["chi2"].any():
            bad.append("chi2")
    d, b = scaled_differences(P, want, got), bounds(rec)
    return bad + ["%s %.3g > %.3g" % (k, d[k], b[k]) for k in FLOAT_OUTPUTS if not d[k] <= b[k]]


# ---------------------------------------------------------------- the independent anchor
ANCHORED = ("chain5", "ring24")


def anchor(name):
    """scipy.optimize.least_squares on the same residuals (sqrt(invSigma2) * error, no kernel) from the same start, over the free
    cameras (an se3 update applied with oplus to the start estimate) and the included points, against the reference run to its stop
    rule.  Returns (the reference's chi2, scipy's, their relative difference)."""
    from scipy.optimize import least_squares
    P = case(name)[0]
    ref = GR.global_bundle_adjustment(P, 200, False)
    assert ref["hits"].get("stopped_by_1e3") or ref["hits"].get("terminate"), "the reference ran out of iterations"
    vertex, edge, included = GR.derive_sets(P)
    role = np.where(vertex == 1, LR.ROLE_LOCAL, LR.ROLE_NONE).astype(np.uint8)
    G = LR.build_graph(P, included, role, edge, LR.REFERENCE, LR.Form())
    sel = np.arange(len(G.k))
    q0, t0 = np.zeros((P.nframes, 4)), np.zeros((P.nframes, 3))
    for f in range(P.nframes):
        E = PR.to_se3(P.Tcw[f])
        q0[f], t0[f] = E.q, E.t
    X0 = P.pos[G.pts].astype(f64)
    nc = len(G.free)

    def residuals(v):
        q, t = q0.copy(), t0.copy()
        for c, f in enumerate(G.free):
            E = PR.oplus(PR.SE3(q0[f], t0[f]), v[6 * c:6 * c + 6])
            q[f], t[f] = E.q, E.t
        _, e0, e1 = LR.project(q, t, X0 + v[6 * nc:].reshape(-1, 3), G, sel)
        s = np.sqrt(G.w)
        return np.concatenate([s * e0, s * e1])
    sol = least_squares(residuals, np.zeros(6 * nc + 3 * len(G.pts)), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=100)
    qf, tf, Xf = ref["estimates"]
    _, e0, e1 = LR.project(qf, tf, Xf, G, sel)
    chi_ref, chi_sp = float(np.sum(PR.edge_chi2(e0, e1, G.w))), float(2.0 * sol.cost)
    return chi_ref, chi_sp, abs(chi_ref - chi_sp) / chi_sp


# ---------------------------------------------------------------- GPU runners
def frames_of(P, ext):
    return [SimpleNamespace(ext=ext, N=len(P.octaves[f]), mvKeysUndistorted=LC.keypoints(P.keys_xy[f], P.octaves[f])) for f in range(P.nframes)]


def result_of(P, poses_in, pose_out, pos, kf_done, point_done, chi2, info, table_after):
    pose_out, poses_in = np.asarray(pose_out), np.asarray(poses_in)
    cam = all(pose_out[k].tobytes() == poses_in[k].tobytes() for k in ("fx", "fy", "cx", "cy", "invfx", "invfy") if k in pose_out.dtype.names)
    return dict(ret=int(info[4]), pose_Tcw=np.array(pose_out["Tcw"], f32).reshape(-1, 12), pose_Ow=np.array(pose_out["Ow"], f32).reshape(-1, 3),
                pos=np.array(pos, f32).reshape(-1, 3), kf_done=np.asarray(kf_done, np.uint8), point_done=np.asarray(point_done, np.uint8),
                chi2=np.asarray(chi2, f32), info=np.asarray(info, np.int32), camera_kept=cam,
                pose_bytes=[pose_out[f].tobytes() for f in range(len(pose_out))], pose_in_bytes=[poses_in[f].tobytes() for f in range(len(poses_in))],
                table=np.array(table_after), all_bytes=pose_out.tobytes() + np.asarray(pos, f32).tobytes() + np.asarray(kf_done).tobytes() +
                np.asarray(point_done).tobytes() + np.asarray(chi2, f32).tobytes() + np.asarray(info, np.int32).tobytes() + np.asarray(table_after).tobytes())


def run_gpu(name, ext):
    """The single call through the Python mirror."""
    from pilotguru_amd.orb import Optimizer
    P, its, robust, in_place = case(name)
    poses, pts = LC.pose_records(P), LC.table(P)
    r = Optimizer.GlobalBundleAdjustment(frames_of(P, ext), poses, pts, P.obs_start, P.obs_frame, P.obs_idx, P.point_bad, P.kf_bad,
                                         P.fixed_id0 if P.fixed_id0.any() else None, its, robust, in_place, ext=ext)
    info = np.array([r["status"], r["edges"], r["included_points"], r["vertices"], r["ret"], r["iterations"], r["trials"], r["envelope"]], np.int32)
    return result_of(P, poses, r["poses"], r["pos"], r["kf_done"], r["point_done"], r["chi2"], info, r["points"])


def device_arrays(P, cap_extra=5):
    """The problem as the device form takes it: (dict of torch tensors, cap, host poses, host table)."""
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    nf = P.nframes
    cap = max(max((len(o) for o in P.octaves), default=0), 1) + cap_extra
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["octave"] = np.nan, np.nan, 99                 # past n: never read
    n = np.zeros(nf, np.int32)
    for f in range(nf):
        m = len(P.octaves[f])
        kp[f, :m] = LC.keypoints(P.keys_xy[f], P.octaves[f])
        n[f] = m
    poses, pts = LC.pose_records(P), LC.table(P)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    D = dict(kps=dev(kp.view(np.uint8).reshape(nf, cap, KEYPOINT_DTYPE.itemsize)), n=dev(n), pose=dev(poses.view(np.uint8).reshape(nf, -1)),
             pts=dev(pts.view(np.uint8).reshape(len(pts), -1)), os=dev(P.obs_start), of=dev(P.obs_frame), oi=dev(P.obs_idx),
             pb=dev(P.point_bad), kb=dev(P.kf_bad), id0=dev(P.fixed_id0) if P.fixed_id0.any() else None)
    return D, cap, poses, pts


def run_gpu_device(name, ext, stream=None, D=None):
    """One call of the device form on resident tensors; returns (result, the tensors, the outputs)."""
    import torch
    from pilotguru_amd.orb import KF_POSE_DTYPE, MAP_POINT_DTYPE, Optimizer
    P, its, robust, in_place = case(name)
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        if D is None:
            D = device_arrays(P)
        T, cap, poses, pts = D
        out = Optimizer.GlobalBundleAdjustment_device(ext, T["kps"], T["n"], cap, T["pose"], len(P.pos), T["pts"], T["os"], T["of"], T["oi"], T["pb"],
                                                      T["kb"], T["id0"], its, robust, in_place, stream=st.cuda_stream)
    st.synchronize()
    po = np.frombuffer(out["pose_out"].cpu().numpy().tobytes(), KF_POSE_DTYPE)
    tb = np.frombuffer(T["pts"].cpu().numpy().tobytes(), MAP_POINT_DTYPE)
    r = result_of(P, poses, po, out["pos_out"].cpu().numpy(), out["kf_done"].cpu().numpy(), out["point_done"].cpu().numpy(),
                  out["chi2"].cpu().numpy(), out["info"].cpu().numpy(), tb)
    return r, D, out
