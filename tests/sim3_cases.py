"""Constructed loop candidates for pgorb_sim3_solver (pilotguru_amd/csrc/sim3.hip) and the runners that put them through the plain
reference (tests/sim3_reference.py), the single call and the batched device form.  A helper module (no tests):
tests/test_sim3_solver.py and tests/golden/make_sim3_spread.py use it.

A scene is two key frames with poses of their own, a true Sim3 S12 between their camera frames, and a map-point table that holds
KF2's points (seen at 2-8 m inside a 640 x 480 image) and KF1's points X1c = s*R*X2c + t, each taken to the world through its key
frame's pose.  Outliers pair a KF2 point with an unrelated KF1 point.  The solver reads only the octaves of the keypoints, so the
keypoint coordinates stay zero.  The draws are chosen on purpose: `draws_for` encodes wanted triples of the compacted order through
the inverse of RandomInt and the swap-with-back list; the rest are random raw values.

The CPU tests hold every case to the case condition (`condition`): the reference run with every error inside the window of its
threshold counted as an inlier, and again as an outlier, must agree in every compared output, and the returned hypothesis must
have no correspondence inside the window."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_reference as SR  # noqa: E402

f32, f64 = np.float32, np.float64
NLEVELS = 8
SIGMA2 = SR.level_sigma2(1.2, NLEVELS)
K1 = (500.0, 500.0, 320.0, 240.0)
K2_OTHER = (430.0, 445.0, 300.0, 255.0)
DEFAULTS = dict(probability=0.99, min_inliers=20, max_iterations=300, fix_scale=0, first_iteration=0, niterations=300, best_inliers_in=0)
MAX_N = 16000
SPREAD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_spread.json")


def rotation(rv):
    rv = np.asarray(rv, f64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def make_pose(R, t, cam):
    T = np.concatenate([np.asarray(R, f64), np.asarray(t, f64).reshape(3, 1)], 1).astype(f32)
    return dict(Tcw=T.reshape(12).copy(), fx=f32(cam[0]), fy=f32(cam[1]), cx=f32(cam[2]), cy=f32(cam[3]))


class Case:
    def __init__(self, name, octaves1, pose1, kf_point1, octaves2, pose2, kf_point2, matches12, points, bad, params, draws, true=None,
                 good=None):
        self.name = name
        self.octaves1, self.octaves2 = np.asarray(octaves1, np.int32), np.asarray(octaves2, np.int32)
        self.pose1, self.pose2 = pose1, pose2
        self.kf_point1, self.kf_point2 = np.asarray(kf_point1, np.int32), np.asarray(kf_point2, np.int32)
        self.matches12 = np.asarray(matches12, np.int32)
        self.points = np.asarray(points, f32).reshape(-1, 3)
        self.bad = None if bad is None else np.asarray(bad, np.uint8)
        self.params = dict(DEFAULTS, **params)
        self.draws = np.asarray(draws, np.uint32).reshape(-1, 3)
        self.true, self.good = true, good                              # the generating (R, t, s); which compacted correspondences are consistent with it

    @property
    def n1(self):
        return len(self.matches12)

    @property
    def n2(self):
        return len(self.kf_point2)

    def variant(self, name=None, params=None, **over):
        """A copy with some fields replaced (the arrays are not copied unless replaced)."""
        f = dict(octaves1=self.octaves1, pose1=self.pose1, kf_point1=self.kf_point1, octaves2=self.octaves2, pose2=self.pose2,
                 kf_point2=self.kf_point2, matches12=self.matches12, points=self.points, bad=self.bad, draws=self.draws)
        f.update(over)
        return Case(name or self.name, f["octaves1"], f["pose1"], f["kf_point1"], f["octaves2"], f["pose2"], f["kf_point2"], f["matches12"],
                    f["points"], f["bad"], dict(self.params, **(params or {})), f["draws"], self.true, self.good)


def encode(index, size):
    """A raw rand() value r with RandomInt(0, size - 1) == index."""
    r = (index * 2 ** 31 + size - 1) // size
    while SR.random_int(r, size) < index:
        r += 1
    assert SR.random_int(r, size) == index and 0 <= r < 2 ** 31
    return r


def draws_for(triples, N, max_iterations, rng):
    """[max_iterations][3] raw values: iteration t takes the compacted correspondences triples[t] (None or past the list: random)."""
    d = rng.randint(0, 2 ** 31, (max_iterations, 3)).astype(np.uint32)
    for t, tri in enumerate(triples):
        if tri is None:
            continue
        avail = list(range(N))
        for i, want in enumerate(tri):
            pos = avail.index(want)
            d[t, i] = encode(pos, len(avail))
            avail[pos] = avail[-1]
            avail.pop()
        assert SR.triple_list(d[t], N) == list(tri)
    return d


def scene(name, seed, n_good, n_out=0, s=1.0, noise=0.0, cam2=K1, octaves="zero", sparse=0, triples=(), params=None, identity_poses=False,
          between=(), one_sided=(), extra=None):
    """n_good consistent and n_out inconsistent correspondences, shuffled; `triples` in terms of ("g", k) = the k-th consistent and
    ("o", k) = the k-th inconsistent correspondence, or plain compacted indices.  sparse: that many further KF1 keypoints that
    drop out (an empty slot, no match, a bad point, in turn).  between: compacted-order ranks of consistent correspondences whose
    KF1 point is moved sideways so that both errors land midway between the truncated and the untruncated threshold; one_sided:
    ranks of those that pass KF1's test and fail KF2's."""
    rng = np.random.RandomState(seed)
    params = dict(params or {})
    N = n_good + n_out
    Rs, ts = rotation(rng.uniform(-0.2, 0.2, 3)), rng.uniform(-0.3, 0.3, 3)
    u, v, z = rng.uniform(60, 580, N), rng.uniform(60, 420, N), rng.uniform(2.0, 8.0, N)
    X2c = np.stack([(u - K1[2]) * z / K1[0], (v - K1[3]) * z / K1[1], z], 1)
    X1c = s * X2c @ Rs.T + ts
    good = np.ones(N, bool)
    good[rng.permutation(N)[:n_out]] = False
    for i in np.nonzero(~good)[0]:                                      # an unrelated KF1 point, far from where S12 puts its partner
        X1c[i] = X1c[i] + np.array([rng.choice([-1, 1]) * rng.uniform(0.4, 1.5), rng.choice([-1, 1]) * rng.uniform(0.4, 1.5), rng.uniform(-0.5, 0.5)]) * s
    if noise:
        X1c[good] += rng.normal(0, noise, (int(good.sum()), 3)) * (X1c[good, 2:3] / K1[0])
    o1 = np.zeros(N, np.int32) if octaves == "zero" else rng.randint(0, NLEVELS, N).astype(np.int32)
    o2 = o1.copy() if octaves == "zero" else rng.randint(0, NLEVELS, N).astype(np.int32)
    gi = np.nonzero(good)[0]
    for k, rank in enumerate(between):                                  # (octaves whose truncation removes more than 1 % of the threshold)
        i = gi[rank]
        o1[i] = o2[i] = (0, 1, 3, 4)[k % 4]
        lo = float(np.floor(9.210 * float(SIGMA2[o1[i]])))
        px = np.sqrt((lo + 9.210 * float(SIGMA2[o1[i]])) / 2.0)
        X1c[i, 0] += px * X1c[i, 2] / K1[0]
    for rank in one_sided:                                              # 4.5 pixels off: below KF1's threshold at octave 4, above KF2's at octave 0
        i = gi[rank]
        o1[i], o2[i] = 4, 0
        X1c[i, 1] += 4.5 * X1c[i, 2] / K1[1]
    if identity_poses:
        R1 = R2 = np.eye(3)
        t1 = t2 = np.zeros(3)
    else:
        R1, t1 = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-2, 2, 3)
        R2, t2 = rotation(rng.uniform(-0.4, 0.4, 3)), rng.uniform(-2, 2, 3)
    P1w, P2w = (X1c - t1) @ R1, (X2c - t2) @ R2
    # the key frames: KF1's keypoints in compacted order with `sparse` drop-outs spread between them; KF2's keypoints permuted
    n1 = N + sparse
    slot_of = np.sort(rng.permutation(n1)[:N])
    perm2 = rng.permutation(N + (3 if sparse else 0))[:N]
    n2 = N + (3 if sparse else 0)
    points = list(P2w) + list(P1w)
    bad = np.zeros(2 * N + sparse + 4, np.uint8)
    kf1, kf2, m12 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32), np.full(n1, -1, np.int32)
    oct1, oct2 = np.zeros(n1, np.int32), np.zeros(n2, np.int32)
    kf2[perm2] = np.arange(N)
    oct2[perm2] = o2
    kf1[slot_of] = N + np.arange(N)
    m12[slot_of] = perm2
    oct1[slot_of] = o1
    spare = [i for i in range(n1) if i not in set(slot_of)]
    for j, i in enumerate(spare):
        kind = j % 3
        if kind == 0 and (j // 3) % 2 == 0:                             # matched, but the KF1 slot is empty
            m12[i] = perm2[j % N]
        elif kind == 0:                                                 # matched to a KF2 keypoint whose slot is empty
            kf1[i] = N + (j % N)
            m12[i] = int(np.nonzero(kf2 < 0)[0][(j // 3) % 3])
        elif kind == 1:                                                 # a point, no match
            kf1[i] = N + (j % N)
        else:                                                           # a match whose KF1 point is bad: a consistent pair that must not count
            points.append(P1w[gi[j % len(gi)]])
            kf1[i] = len(points) - 1
            bad[kf1[i]] = 1
            m12[i] = perm2[gi[j % len(gi)]]
    points = np.array(points, f64)
    if extra:
        extra(locals())
    go = [int(k) for k in np.nonzero(good)[0]]
    oo = [int(k) for k in np.nonzero(~good)[0]]
    tri = [None if t is None else [go[k[1]] if isinstance(k, tuple) and k[0] == "g" else oo[k[1]] if isinstance(k, tuple) else int(k) for k in t]
           for t in triples]
    draws = draws_for(tri, N, int(dict(DEFAULTS, **params)["max_iterations"]), rng)
    return Case(name, oct1, make_pose(R1, t1, K1), kf1, oct2, make_pose(R2, t2, cam2), kf2, m12, points.astype(f32),
                bad[:len(points)] if sparse else None, params, draws, true=(Rs, ts, s), good=good)


def _degenerate():
    """Iteration 0: three correspondences whose two clouds are identical (the same table point through the same pose), so M is
    symmetric, the quaternion is (1, 0, 0, 0), norm(vec) == 0 and everything after it is NaN.  Iteration 1: three collinear
    correspondences.  Iteration 2: a triple with the correspondence whose KF1 point lies at z = 0 (its image is not finite, so it is
    never an inlier).  Iteration 3: a clean triple."""
    def extra(L):
        N, pts, X2c, X1c, good = L["N"], L["points"], L["X2c"], L["X1c"], L["good"]
        oo = np.nonzero(~good)[0]
        for k in oo[:3]:                                                # identical clouds: KF1's slot names KF2's own point
            pts[N + k] = pts[k]
        a, b = oo[3], oo[4]
        go = np.nonzero(good)[0]
        g0, g1 = go[0], go[1]                                           # collinear: two consistent pairs and a pair on the line through them, in both clouds
        pts[b] = 0.35 * pts[g0] + 0.65 * pts[g1]
        pts[N + b] = 0.35 * pts[N + g0] + 0.65 * pts[N + g1]
        pts[N + a, 2] = 0.0                                             # z = 0 in KF1's camera frame (identity pose)
    return scene("degenerate_triples", 77, 30, 6, s=1.2, identity_poses=True, extra=extra,
                 triples=[[("o", 0), ("o", 1), ("o", 2)], [("g", 0), ("g", 1), ("o", 4)], [("o", 3), ("g", 2), ("g", 3)],
                          [("g", 4), ("g", 9), ("g", 17)]])


def single_cases():
    out_first = [[("o", 0), ("g", 0), ("g", 1)], [("g", 2), ("o", 1), ("o", 2)], [("g", 3), ("g", 4), ("o", 3)], [("g", 0), ("g", 5), ("g", 11)]]
    cs = [
        scene("few_19", 1, 19),
        scene("n20_cap_one", 2, 20, triples=[[("g", 0), ("g", 7), ("g", 13)]]),
        scene("n21_clean", 3, 21, triples=[[("g", 20), ("g", 3), ("g", 11)]]),
        scene("n64_outliers", 4, 45, 19, triples=out_first),
        scene("n65_outliers", 5, 46, 19, triples=out_first),
        scene("n257_outliers", 6, 180, 77, triples=out_first),
        # 16 consistent pairs of 40: no hypothesis reaches 21; two clean triples tie at the maximum and `best` is the later one
        scene("heavy_outliers", 7, 16, 24, noise=0.05, triples=[None] * 5 + [[("g", 0), ("g", 6), ("g", 12)]] + [None] * 20 + [[("g", 1), ("g", 7), ("g", 15)]]),
        scene("scale_free", 8, 30, 6, s=1.7, triples=[[("g", 0), ("o", 0), ("g", 1)], [("g", 2), ("g", 12), ("g", 25)]]),
        scene("scale_fixed", 8, 30, 6, s=1.7, triples=[[("g", 0), ("o", 0), ("g", 1)], [("g", 2), ("g", 12), ("g", 25)]], params=dict(fix_scale=1)),
        scene("scale_fixed_unit", 9, 30, 6, s=1.0, triples=[[("g", 0), ("o", 0), ("g", 1)], [("g", 2), ("g", 12), ("g", 25)]], params=dict(fix_scale=1)),
        scene("two_cameras", 10, 40, 10, s=1.1, cam2=K2_OTHER, triples=[[("o", 0), ("o", 1), ("g", 1)], [("g", 2), ("g", 22), ("g", 35)]]),
        scene("mixed_octaves", 11, 48, 12, octaves="mixed", between=(5, 9, 14, 20, 26, 31, 37, 41), one_sided=(7, 16, 33), triples=[[("o", 0), ("g", 0), ("g", 1)], [("g", 2), ("g", 23), ("g", 40)]]),
        scene("sparse_slots", 12, 44, 12, sparse=23, triples=[[("o", 0), ("g", 0), ("g", 1)], [("g", 2), ("g", 21), ("g", 38)]]),
        _degenerate(),
        # seven triples with an outlier each, then a clean one: the success lies in the second window of five
        scene("late_success", 14, 40, 15, triples=[[("o", k), ("g", k), ("g", k + 1)] for k in range(7)] + [[("g", 3), ("g", 19), ("g", 33)]]),
    ]
    # one draw at 2^31 - 1: RandomInt gives the last position of the list
    c = cs[2]
    c.draws[0, 0] = 2 ** 31 - 1
    # a resumed solver: mnIterations = 1 and a carried best above what iteration 1 reaches
    cs.append(resume_case())
    return cs


def resume_case():
    """Iteration 1 fits through a correspondence that lies several pixels off: more than min_inliers agree, fewer than the best
    carried in from an earlier call; it is passed over and iteration 2, a clean triple, returns.  The offset is the first of a
    fixed list that leaves iteration 1 between 25 and 45 inliers."""
    for px in (4.0, 6.0, 8.0, 10.0, 12.0, 16.0, 24.0):
        def extra(L):
            X1c, good, pts, N, R1, t1 = L["X1c"], L["good"], L["points"], L["N"], L["R1"], L["t1"]
            g = np.nonzero(good)[0][3]
            x = X1c[g] + np.array([px * X1c[g, 2] / K1[0], 0.0, 0.0])
            pts[N + g] = (x - t1) @ R1
        c = scene("resume_carried_best", 13, 50, 15, extra=extra, params=dict(first_iteration=1, best_inliers_in=48),
                  triples=[[("o", 0), ("o", 1), ("g", 0)], [("g", 3), ("g", 1), ("g", 2)], [("g", 5), ("g", 25), ("g", 44)]])
        tr = []
        run_reference(c, trace=tr, niterations=1, best_inliers_in=0)
        if 25 <= tr[0][5] <= 45:
            return c
    raise AssertionError("resume_carried_best: no offset leaves iteration 1 between 25 and 45 inliers")


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = single_cases()
    return _CASES


def case(name):
    return next(c for c in all_cases() if c.name == name)


# ---------------------------------------------------------------- the reference
def run_reference(c, rules=SR.REFERENCE, forms=SR.READING, near=None, window=0.0, trace=None, **kw):
    return SR.sim3_solver(c.octaves1, c.pose1, c.kf_point1, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.points, c.bad, SIGMA2,
                          dict(c.params, **kw), c.draws, rules, forms, near, window, trace)


_REF = {}


def reference(c):
    """The reference's result for a case, computed once and shared (callers must not change it)."""
    if c.name not in _REF:
        _REF[c.name] = run_reference(c)
    return _REF[c.name]


# ---------------------------------------------------------------- tolerances (tests/golden/sim3_spread.json)
FLOAT_OUTPUTS = ("R", "t", "s", "err")
INT_FIELDS = ("ret", "status", "N", "cap", "its_after", "ninliers", "best_inliers", "best_iteration", "inlier", "matches12_out", "already1",
              "already2")
ULP1 = float(np.spacing(f32(1.0)))


def _nan_equal_diff(a, b):
    """max |a - b| over entries where either is finite; an entry that is NaN (or the same infinity) in both counts as equal, one
    that is finite in one only as infinitely different."""
    a, b = np.asarray(a, f64).reshape(-1), np.asarray(b, f64).reshape(-1)
    with np.errstate(all="ignore"):
        same = (np.isnan(a) & np.isnan(b)) | (a == b)
        d = np.where(same, 0.0, np.abs(a - b))
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if len(d) else 0.0


def scaled_differences(a, b):
    """The largest difference per float output between two results: rotation entries as they are, t by max(1, |t|inf), s by
    max(1, s), each over `found` (with the pgorb_sim3 record: sR by max(1, s), 1/s * R.t() by max(1, 1/s)) and `best`."""
    out = dict(R=0.0, t=0.0, s=0.0)
    for pre in ("found_", "best_"):
        ts = max(1.0, float(np.nanmax(np.abs(np.asarray(a[pre + "t"], f64))))) if np.isfinite(a[pre + "t"]).any() else 1.0
        ss = max(1.0, abs(float(a[pre + "s"]))) if np.isfinite(a[pre + "s"]) else 1.0
        out["R"] = max(out["R"], _nan_equal_diff(a[pre + "R"], b[pre + "R"]))
        out["t"] = max(out["t"], _nan_equal_diff(a[pre + "t"], b[pre + "t"]) / ts)
        out["s"] = max(out["s"], _nan_equal_diff([a[pre + "s"]], [b[pre + "s"]]) / ss)
    s = abs(float(a["found_s"]))
    if s > 0 and np.isfinite(s):
        ts = max(1.0, float(np.abs(np.asarray(a["found_t"], f64)).max()))
        t21s = max(1.0, float(np.abs(np.asarray(a["t21"], f64)).max()))
        out["R"] = max(out["R"], _nan_equal_diff(a["sR12"], b["sR12"]) / max(1.0, s), _nan_equal_diff(a["sR21"], b["sR21"]) / max(1.0, 1.0 / s))
        out["t"] = max(out["t"], _nan_equal_diff(a["t12"], b["t12"]) / ts, _nan_equal_diff(a["t21"], b["t21"]) / t21s)
    return out


def returned_errors(c, forms):
    """err1, err2 of every correspondence under the hypothesis a call ends with (found, else best), and the thresholds."""
    tr = []
    r = run_reference(c, forms=forms, trace=tr)
    it = r["best_iteration"]
    if it < 0:
        return r, None
    t, tri, T, e1, e2, inl = next(x for x in tr if x[0] == it)
    return r, (e1, e2)


def spread(c):
    """The largest scaled difference per output between the reference's arithmetic forms.  err: |difference| / max(threshold, err)
    over the correspondences of the hypothesis the call ends with.  Raises when the forms do not agree in an integer output: such
    a case decides nothing and has to be rebuilt."""
    C0 = SR.correspondences(c.octaves1, c.pose1, c.kf_point1, c.octaves2, c.pose2, c.kf_point2, c.matches12, c.points, c.bad, SIGMA2)
    rs = {k: returned_errors(c, f) for k, f in SR.FORMS.items()}
    names = list(rs)
    out = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            (a, ea), (b, eb) = rs[names[i]], rs[names[j]]
            bad = [k for k in INT_FIELDS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
            if bad:
                raise AssertionError("%s: forms %s and %s differ in %s" % (c.name, names[i], names[j], bad))
            d = scaled_differences(a, b)
            for k in ("R", "t", "s"):
                out[k] = max(out[k], d[k])
            if ea is not None:
                for x, y, th in ((ea[0], eb[0], C0.th1), (ea[1], eb[1], C0.th2)):
                    with np.errstate(all="ignore"):
                        sc = np.maximum(th.astype(f64), np.where(np.isfinite(x), np.abs(x.astype(f64)), 0.0))
                        fin = np.isfinite(x) | np.isfinite(y)
                        dd = np.where(fin, np.abs(x.astype(f64) - y.astype(f64)) / sc, 0.0)
                    dd = np.where(np.isnan(dd), np.inf, dd)
                    out["err"] = max(out["err"], float(dd.max()) if len(dd) else 0.0)
    return out


def recorded_spread():
    with open(SPREAD_FILE) as f:
        return json.load(f)


def bounds(recorded):
    """The bound per output: the larger of 2 float ulps at the scale (the differences are scaled to 1) and 16 x the recorded spread.
    The floor is there because the results are floats: two doubles 1e-12 apart can land on neighbouring floats.  The factor covers
    that the device's atan2, sin and cos differ from the host's in the last place."""
    return {k: max(2.0 * ULP1, 16.0 * float(recorded[k])) for k in ("R", "t", "s")}


def window(recorded):
    """The classification window of the case condition, relative to a threshold: 16 x the recorded relative spread of err, with a
    floor of 4 float ulps."""
    return max(4.0 * ULP1, 16.0 * float(recorded["err"]))


def condition(c, recorded):
    """The case condition; returns the list of what fails (empty = the case decides)."""
    w = window(recorded)
    a, b = run_reference(c, near="in", window=w), run_reference(c, near="out", window=w)
    bad = [k for k in INT_FIELDS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    for k in ("found_R", "found_t", "found_s", "best_R", "best_t", "best_s", "sR12", "t12", "sR21", "t21"):
        if np.asarray(a[k], f32).tobytes() != np.asarray(b[k], f32).tobytes():
            bad.append(k)
    if a["near_found"] or b["near_found"]:
        bad.append("%d correspondences of the returned hypothesis inside the window" % max(a["near_found"], b["near_found"]))
    return bad


def differences(c, want, got, recorded):
    """The compared outputs that differ: integers and flags exactly, floats by bounds(); what is zeroed must be zero bytes."""
    bad = [k for k in INT_FIELDS if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]
    d, b = scaled_differences(want, got), bounds(recorded)
    bad += ["%s %.3g > %.3g" % (k, d[k], b[k]) for k in ("R", "t", "s") if not d[k] <= b[k]]
    if not want["status"] & SR.S3_FOUND:
        for k in ("found_R", "found_t", "found_s", "sR12", "t12", "sR21", "t21"):
            if np.asarray(got[k]).any():
                bad.append(k + " not zeroed")
    return bad, d


# ---------------------------------------------------------------- GPU runners
def table(points):
    from pilotguru_amd.orb import MAP_POINT_DTYPE
    pts = np.zeros(max(len(points), 1), MAP_POINT_DTYPE)
    pts["pos"][:len(points)] = points
    return pts


def keypoints(octaves):
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(max(len(octaves), 1), KEYPOINT_DTYPE)
    k["octave"][:len(octaves)] = octaves
    return k


def pose_record(pose):
    from pilotguru_amd.orb import kf_pose
    return kf_pose(np.asarray(pose["Tcw"], f32).reshape(3, 4), np.zeros(3, f32), pose["fx"], pose["fy"], pose["cx"], pose["cy"])


def params_record(prm):
    from pilotguru_amd.orb import SIM3_PARAMS_DTYPE
    r = np.zeros(1, SIM3_PARAMS_DTYPE)
    for k in DEFAULTS:
        r[k] = prm[k]
    return r


def result_of(ret, found, sim3, best, inlier, mout, a1, a2, info):
    return dict(ret=int(ret), status=int(info[0]), N=int(info[1]), cap=int(info[2]), its_after=int(info[3]), ninliers=int(info[4]),
                best_inliers=int(info[5]), best_iteration=int(info[6]),
                found_R=np.array(found["R12"], f32).reshape(9), found_t=np.array(found["t12"], f32).reshape(3), found_s=f32(found["s12"]),
                best_R=np.array(best["R12"], f32).reshape(9), best_t=np.array(best["t12"], f32).reshape(3), best_s=f32(best["s12"]),
                sR12=np.array(sim3["sR12"], f32).reshape(9), t12=np.array(sim3["t12"], f32).reshape(3),
                sR21=np.array(sim3["sR21"], f32).reshape(9), t21=np.array(sim3["t21"], f32).reshape(3),
                inlier=np.asarray(inlier, np.uint8).copy(), matches12_out=np.asarray(mout, np.int32).copy(),
                already1=np.asarray(a1, np.uint8).copy(), already2=np.asarray(a2, np.uint8).copy(),
                raw=b"".join(np.ascontiguousarray(x).tobytes() for x in (found, sim3, best, inlier, mout, a1, a2, np.asarray(info[:7]))))


def run_gpu(c, ext, **kw):
    """The single call through the C ABI."""
    from pilotguru_amd.orb import SIM3_DTYPE, SIM3_ESTIMATE_DTYPE
    L, h = ext._L, ext._h
    n1, n2 = c.n1, c.n2
    k1, k2, pts = keypoints(c.octaves1), keypoints(c.octaves2), table(c.points)
    P1, P2 = np.asarray(pose_record(c.pose1)).reshape(1), np.asarray(pose_record(c.pose2)).reshape(1)
    prm = params_record(dict(c.params, **kw))
    found, best, sim3 = np.zeros(1, SIM3_ESTIMATE_DTYPE), np.zeros(1, SIM3_ESTIMATE_DTYPE), np.zeros(1, SIM3_DTYPE)
    found["s12"] = best["s12"] = 9
    fl, mo, a1, a2 = np.full(max(n1, 1), 9, np.uint8), np.full(max(n1, 1), -9, np.int32), np.full(max(n1, 1), 9, np.uint8), np.full(max(n2, 1), 9, np.uint8)
    info = np.full(8, -9, np.int32)
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    kf1, kf2, m12, draws = (np.ascontiguousarray(x) for x in (c.kf_point1, c.kf_point2, c.matches12, c.draws))
    ret = L.pgorb_sim3_solver(h, p(k1), n1, p(P1), p(kf1), p(k2), n2, p(P2), p(kf2), p(m12), len(c.points), p(pts), p(c.bad), p(prm), p(draws),
                              p(found), p(sim3), p(best), p(fl), p(mo), p(a1), p(a2), p(info))
    if ret < 0:
        return ret
    return result_of(ret, found[0], sim3[0], best[0], fl[:n1], mo[:n1], a1[:n1], a2[:n2], info)


def batch_groups(cases):
    """The cases grouped by what one batched call shares: everything in the parameter block but first_iteration and
    best_inliers_in, which go per pair."""
    groups = {}
    for c in cases:
        key = tuple(c.params[k] for k in ("probability", "min_inliers", "max_iterations", "fix_scale", "niterations"))
        groups.setdefault(key, []).append(c)
    return list(groups.values())


def run_gpu_batch(cases, ext, cap, order=None, stream=None):
    """One launch of pgorb_sim3_solver_batch_device over `cases` (one group of batch_groups) in `order`, every key frame padded to
    `cap`; the map-point tables are concatenated.  Returns the per-pair results in that order."""
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE, KF_POSE_DTYPE, SIM3_DTYPE, SIM3_ESTIMATE_DTYPE, MAP_POINT_DTYPE
    L, h = ext._L, ext._h
    order = list(range(len(cases))) if order is None else list(order)
    cs = [cases[j] for j in order]
    npair, nf = len(cs), 2 * len(cs)
    maxits = int(cs[0].params["max_iterations"])
    kp = np.zeros((nf, cap), KEYPOINT_DTYPE)
    kp["octave"] = 99                                                   # past n: never read
    slots = np.full((nf, cap), 1 << 20, np.int32)
    m12 = np.full((npair, cap), 12345, np.int32)
    n = np.zeros(nf, np.int32)
    poses = np.zeros(nf, KF_POSE_DTYPE)
    draws = np.zeros((npair, maxits, 3), np.uint32)
    base, tabs, bads = 0, [], []
    for j, c in enumerate(cs):
        kp[2 * j, :c.n1] = keypoints(c.octaves1)[:c.n1]
        kp[2 * j + 1, :c.n2] = keypoints(c.octaves2)[:c.n2]
        slots[2 * j, :c.n1] = np.where(c.kf_point1 >= 0, c.kf_point1 + base, -1)
        slots[2 * j + 1, :c.n2] = np.where(c.kf_point2 >= 0, c.kf_point2 + base, -1)
        m12[j, :c.n1] = c.matches12
        n[2 * j], n[2 * j + 1] = c.n1, c.n2
        poses[2 * j], poses[2 * j + 1] = pose_record(c.pose1), pose_record(c.pose2)
        draws[j] = c.draws
        tabs.append(table(c.points)[:len(c.points)])
        bads.append(np.zeros(len(c.points), np.uint8) if c.bad is None else c.bad)
        base += len(c.points)
    tab, bad = np.concatenate(tabs), np.concatenate(bads)
    st = torch.cuda.current_stream() if stream is None else stream
    keep = []

    def p(t):
        keep.append(t)
        return C.c_void_p(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    prm = params_record(cs[0].params)
    with torch.cuda.stream(st):
        dk, dn, dpo, dsl, dm = dev(kp), dev(n), dev(poses), dev(slots), dev(m12)
        d1, d2 = dev(np.arange(0, nf, 2, dtype=np.int32)), dev(np.arange(1, nf, 2, dtype=np.int32))
        dt, db, dd = dev(tab), dev(bad), dev(draws)
        dfi = dev(np.array([c.params["first_iteration"] for c in cs], np.int32))
        dbi = dev(np.array([c.params["best_inliers_in"] for c in cs], np.int32))
        full = lambda shape, dt_: torch.full(shape, 77, dtype=dt_, device="cuda")
        o_f, o_b = full((npair, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8), full((npair, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8)
        o_s = full((npair, SIM3_DTYPE.itemsize), torch.uint8)
        o_in, o_a1, o_a2 = full((npair, cap), torch.uint8), full((npair, cap), torch.uint8), full((npair, cap), torch.uint8)
        o_mo, o_info, o_ni = full((npair, cap), torch.int32), full((npair, 8), torch.int32), full((npair,), torch.int32)
        ext._check(L.pgorb_sim3_solver_batch_device(h, p(dk), p(dn), cap, p(d1), p(d2), npair, p(dpo), p(dsl), p(dm), len(tab), p(dt), p(db),
                                                    prm.ctypes.data_as(C.c_void_p), p(dfi), p(dbi), p(dd), p(o_f), p(o_s), p(o_b), p(o_in), p(o_mo),
                                                    p(o_a1), p(o_a2), p(o_info), p(o_ni), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    found = np.frombuffer(o_f.cpu().numpy().tobytes(), SIM3_ESTIMATE_DTYPE)
    best = np.frombuffer(o_b.cpu().numpy().tobytes(), SIM3_ESTIMATE_DTYPE)
    sim3 = np.frombuffer(o_s.cpu().numpy().tobytes(), SIM3_DTYPE)
    fl, mo, a1, a2, info, ni = (t.cpu().numpy() for t in (o_in, o_mo, o_a1, o_a2, o_info, o_ni))
    res = []
    for j, c in enumerate(cs):
        r = result_of(ni[j], found[j], sim3[j], best[j], fl[j, :c.n1], mo[j, :c.n1], a1[j, :c.n1], a2[j, :c.n2], info[j])
        # every entry of a row is written: past n there is no correspondence
        r["tail_ok"] = bool((fl[j, c.n1:] == 0).all() and (mo[j, c.n1:] == -1).all() and (a1[j, c.n1:] == 0).all() and (a2[j, c.n2:] == 0).all())
        res.append(r)
    return res


# ---------------------------------------------------------------- the chain of ComputeSim3: SearchByBoW -> Sim3Solver -> SearchBySim3
CHAIN_SEEDS = (21, 22, 23)
CHAIN_TH = 7.5


def chain_pair(seed):
    """A pair_case of tests/loop_cases.py (two key frames of about 120 keypoints whose maps differ by a Sim3) prepared for the whole
    chain: the physical pairing of the two maps' points is recovered through the generating Sim3; a keypoint that holds a point
    gets the vocabulary node of its physical point, and for most pairs KF2's keypoint gets a descriptor a few bits from KF1's, so
    that SearchByBoW finds them; a few KF2 keypoints get the descriptor of ANOTHER pair of the same node (wrong matches: the
    solver's outliers).  Returns (PairCase, BowCase, draws)."""
    import loop_cases as LC
    c = LC.pair_case(seed, npts=105, s12=(1.0, 1.25, 0.85)[seed % 3])
    rng = np.random.RandomState(900 + seed)
    T1, T2 = (np.asarray(k[2]["Tcw"], f64).reshape(3, 4) for k in (c.kf1, c.kf2))
    sR12, t12 = np.asarray(c.sim3["sR12"], f64).reshape(3, 3), np.asarray(c.sim3["t12"], f64)
    pos = np.array([p["pos"] for p in c.points], f64)
    in1 = np.zeros(len(pos), bool)
    in1[c.slots1[c.slots1 >= 0]] = True
    X1 = pos @ T1[:, :3].T + T1[:, 3]
    X2in1 = (pos @ T2[:, :3].T + T2[:, 3]) @ sR12.T + t12
    partner = {}                                                        # KF2's point -> KF1's point of the same physical point
    for q in c.slots2[c.slots2 >= 0]:
        d = np.linalg.norm(X1 - X2in1[q], axis=1) + np.where(in1, 0.0, 1e9)
        if d.min() < 1e-3:
            partner[int(q)] = int(d.argmin())
    holder1 = {int(s): i for i, s in enumerate(c.slots1) if s >= 0}
    k1, d1, P1 = c.kf1
    k2, d2, P2 = c.kf2
    d2 = d2.copy()
    nodes1, nodes2 = rng.randint(100, 200, len(k1)), rng.randint(200, 300, len(k2))      # keypoints without a pair share no node
    pairs = []
    for i2, q in enumerate(c.slots2):
        if int(q) in partner:
            i1 = holder1[partner[int(q)]]
            nodes1[i1] = nodes2[i2] = partner[int(q)] % 7
            pairs.append((i1, i2))
            if rng.rand() < 0.8:
                d2[i2] = LC.at_distance(d1[i1], int(rng.randint(0, 25)), rng)
    for k in range(0, len(pairs) - 1, 9):                               # a wrong match: KF2's keypoint looks like another pair's KF1 keypoint
        (i1, i2), (j1, j2) = pairs[k], pairs[k + 1]
        nodes2[i2] = nodes1[j1]
        d2[i2] = LC.at_distance(d1[j1], 1, rng)
        d2[j2] = LC.at_distance(d1[j1], 60, rng)
    bad = np.array([bool(p.get("bad", False)) for p in c.points])
    valid = lambda sl: np.array([s >= 0 and not bad[s] for s in sl], np.uint8)  # noqa: E731
    c = LC.PairCase("chain%d" % seed, (k1, d1, P1), (k2, d2, P2), c.points, c.slots1, c.slots2, c.sim3, c.already1, c.already2, CHAIN_TH)
    b = LC.BowCase("chain%d" % seed, d1, k1["angle"], valid(c.slots1), nodes1, d2, k2["angle"], valid(c.slots2), nodes2)
    draws = rng.randint(0, 2 ** 31, (DEFAULTS["max_iterations"], 3)).astype(np.uint32)
    return c, b, draws


def chain_solver_case(c, m12, draws):
    """The solver's problem after SearchByBoW gave m12 on the pair case c."""
    pose = lambda P: dict(Tcw=np.array(P["Tcw"], f32), fx=f32(P["fx"]), fy=f32(P["fy"]), cx=f32(P["cx"]), cy=f32(P["cy"]))  # noqa: E731
    return Case("solver_" + c.name, c.kf1[0]["octave"], pose(c.kf1[2]), c.slots1, c.kf2[0]["octave"], pose(c.kf2[2]), c.slots2, m12,
                np.array([p["pos"] for p in c.points], f32), np.array([bool(p.get("bad", False)) for p in c.points], np.uint8), {}, draws)


def chain_reference(seed):
    """The chain through the references: (pair case, bow case, draws, m12, solver case, solver result, (nFound, match12))."""
    import loop_cases as LC
    import loop_reference as LR
    import pilotguru_amd as pg
    c, b, draws = chain_pair(seed)
    _, m12 = LC.run_ref1(b)
    sc = chain_solver_case(c, m12, draws)
    r = run_reference(sc)
    sim3 = pg.sim3_record(r["sR12"], r["t12"], r["sR21"], r["t21"])
    kf1, kf2 = c.build()
    n3, s12 = LR.search_by_sim3(kf1, kf2, sim3, list(r["already1"]), list(r["already2"]), c.th)
    return c, b, draws, m12, sc, r, (n3, np.array(s12, np.int32))
