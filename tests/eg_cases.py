"""Constructed essential graphs for tests/test_optimize_essential_graph.py: the smallest graphs at which each part of
pgorb_optimize_essential_graph can go wrong.  A helper module (no tests).

A world is n key frames on a ring (generating Sim3 G_i, world -> camera) whose estimated poses drift along the ride (G_i * D_i,
D_i = exp(xi * i / n)); the loop is closed between the last key frame (cur) and the first (loop).  CorrectedSim3 holds the
generating Sim3 of cur and its neighbour, NonCorrectedSim3 their drifted poses, as LoopClosing::CorrectLoop leaves them.  The four
candidate lists hold what the containers would hold, survivors and rejects alike.  `case(name)` returns the dict that
eg_reference.optimize_essential_graph and the library's mirrors read; `bounds(name)` the comparison bounds from
tests/golden/eg_spread.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eg_reference as ER  # noqa: E402
from optsim3_reference import Sim3, sim3_exp, sim3_inverse, sim3_mul  # noqa: E402
from pose_reference import matrix_from_quat, quat_from_matrix  # noqa: E402

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
SPREAD_PATH = os.path.join(HERE, "golden", "eg_spread.json")
KF_POSE_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                          ("invfx", "<f4"), ("invfy", "<f4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4")])
SIM3D_DTYPE = np.dtype([("r", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
LM = ER.LibM2(False)
FLOAT_OUTPUTS = ("Tcw", "Ow", "pos")
DOUBLE_OUTPUTS = ("sim3", "rel", "chi2")


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def record(S):
    r = np.zeros((), SIM3D_DTYPE)
    r["r"], r["t"], r["s"] = S.q, S.t, S.s
    return r


def pose_record(S):
    """The key frame's float pose of a Sim3: [R | t/s], Ow = -R't, a camera."""
    P = np.zeros((), KF_POSE_DTYPE)
    R = matrix_from_quat(S.q)
    t = S.t / S.s
    P["Tcw"] = np.concatenate([R, t.reshape(3, 1)], 1).reshape(12).astype(f32)
    P["Ow"] = (-R.T @ t).astype(f32)
    P["fx"], P["fy"], P["cx"], P["cy"] = 500.0, 510.0, 320.0, 240.0
    P["invfx"], P["invfy"] = f32(1.0) / f32(500.0), f32(1.0) / f32(510.0)
    return P


def world(n, seed, xi_scale=1.0, sigma=0.04):
    """(G [n], drifted [n]): the generating Sim3s and G_i * exp(xi * i / n)."""
    rng = np.random.RandomState(seed)
    xi = np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.25, 0.25, 3), [sigma]]) * xi_scale
    G, D = [], []
    for i in range(n):
        a = 2 * np.pi * i / (n + 1)
        c = np.array([6.0 * np.cos(a), 0.3 * np.sin(3 * a), 6.0 * np.sin(a)]) + rng.uniform(-0.1, 0.1, 3)
        R = _rot(-a + rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
        g = Sim3(quat_from_matrix(R), -R @ c, 1.0)
        G.append(g)
        D.append(sim3_mul(g, sim3_exp(xi * (i / float(n)), LM)))
    return G, D


def _csr(rows):
    start = np.zeros(len(rows) + 1, np.int32)
    start[1:] = np.cumsum([len(r) for r in rows])
    flat = [x for r in rows for x in r]
    return start, flat


def build(n, seed, fix_scale=0, covis_back=2, loop_conn=None, loop_edges=None, covis_extra=None, parent=None, kf_bad=(), corrected=(-1, -2),
          all_maps=False, no_maps=False, xi_scale=1.0, min_feat=100, iterations=20, ids=None, sigma=0.04):
    G, D = world(n, seed, xi_scale, 0.0 if fix_scale else sigma)
    cur, loop = n - 1, 0
    c = dict(nkf=n, loop_kf=loop, cur_kf=cur, fix_scale=int(fix_scale), min_feat=min_feat, iterations=iterations)
    c["kf_id"] = np.asarray(ids if ids is not None else 3 * np.arange(n) + 7, np.uint64)
    c["pose"] = np.array([pose_record(D[i]) for i in range(n)], KF_POSE_DTYPE)
    bad = np.zeros(n, np.uint8)
    bad[list(kf_bad)] = 1
    c["kf_bad"] = bad
    hc, hn = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    cor, non = np.zeros(n, SIM3D_DTYPE), np.zeros(n, SIM3D_DTYPE)
    cor["r"][:, 3] = non["r"][:, 3] = 1.0
    cor["s"] = non["s"] = 1.0
    if all_maps:                                    # every vertex from CorrectedSim3, every normal edge from a consistent NonCorrectedSim3
        K = sim3_exp(np.array([0.02, -0.01, 0.03, 0.2, -0.1, 0.3, 0.0 if fix_scale else 0.1]), LM)
        for i in range(n):
            hc[i] = hn[i] = 1
            cor[i] = record(G[i] if i in (cur, loop) else D[i])
            non[i] = record(sim3_mul(G[i], K))
    elif not no_maps:
        for k in corrected:
            i = k % n
            hc[i] = hn[i] = 1
            cor[i] = record(G[i])
            non[i] = record(Sim3(D[i].q, D[i].t / D[i].s, 1.0))
    c.update(has_corrected=hc, corrected=cor, has_non_corrected=hn, non_corrected=non)
    c["loop_conn"] = np.asarray([(cur, loop, 60)] if loop_conn is None else loop_conn, np.int32).reshape(-1, 3)
    c["parent"] = np.asarray(parent if parent is not None else [-1] + list(range(n - 1)), np.int32)
    c["loop_edge_start"], c["loop_edge"] = _csr(loop_edges if loop_edges is not None else [[] for _ in range(n)])
    cv = [[(i - k, 100 + 7 * k + i) for k in range(1, covis_back + 1) if i - k >= 0] + [(i + 1, 150)] * (1 if i + 1 < n else 0) for i in range(n)]
    for i, lst in (covis_extra or {}).items():
        cv[i] = list(lst) + cv[i]
    c["covis_start"], flat = _csr(cv)
    c["covis"], c["covis_weight"] = [x[0] for x in flat], [x[1] for x in flat]
    for k in ("loop_edge", "covis", "covis_weight"):
        c[k] = np.asarray(c[k], np.int32).reshape(-1)
    # the points: three per key frame in front of its drifted camera, then one without a reference key frame and one bad point
    rng = np.random.RandomState(seed + 1000)
    pts, ref = [], []
    for i in range(n):
        Swc = sim3_inverse(D[i])
        for _ in range(3):
            pc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 8)])
            pts.append(ER.sim3_map(Swc, pc))
            ref.append(i)
    pts += [np.array([0.5, -0.25, 1.5]), np.array([1.0, 2.0, 3.0])]
    ref += [-1, cur]
    P = np.zeros(len(pts), MAP_POINT_DTYPE)
    P["pos"] = np.asarray(pts, f32)
    P["normal"] = rng.uniform(-1, 1, (len(pts), 3)).astype(f32)
    P["min_distance"], P["max_distance"] = 0.5, 20.0
    pb = np.zeros(len(pts), np.uint8)
    pb[-1] = 1
    c.update(points=P, point_bad=pb, point_ref_kf=np.asarray(ref, np.int32), G=G, D=D)
    return c


def _filters():
    """Every filter once, on a ring of 12 (cur = 11, loop = 0)."""
    n = 12
    loop_edges = [[] for _ in range(n)]
    loop_edges[9] = [2, 10]              # 2: a smaller mnId, an edge; 10: a larger one, none (:930)
    loop_edges[2] = [9]                  # the other direction of the same previous loop: a larger mnId
    loop_edges[10] = [9]
    extra = {
        9: [(2, 300),                    # a covisible that is a loop edge of 9: none
            (8, 250),                    # its parent: none
            (10, 240),                   # its child (and a larger mnId): none
            (5, 99), (6, 100),           # weight 99: none; weight 100: an edge
            (11, 500)],                  # a larger mnId: none
        11: [(0, 400), (1, 130), (3, 99)],   # (11, 0) and (11, 1) are in sInsertedEdges: none
        4: [(1, 100)],
        7: [(3, 200)],                   # key frame 3 hangs under 7 (ChangeParent after a culling): a child with a smaller mnId, none
    }
    parent = [-1] + list(range(n - 1))
    parent[3] = 7
    lc = [(11, 0, 10),                   # (cur, loop): kept below minFeat
          (11, 1, 100),                  # weight 100: kept
          (11, 2, 99),                   # weight 99: skipped
          (10, 0, 10),                   # not (cur, loop), below minFeat: skipped
          (0, 11, 10),                   # (loop, cur) is not the exception: skipped
          (1, 10, 120)]                  # the set of key frame 1, a smaller index first
    return build(n, 21, loop_conn=lc, loop_edges=loop_edges, covis_extra=extra, parent=parent)


def _isolated():
    n = 12
    parent = [-1] + list(range(n - 1))
    parent[5], parent[6] = -1, 4
    c = build(n, 22, covis_back=0, parent=parent)
    # no covisible names key frame 5 and it names none
    keep = [[(int(c["covis"][k]), int(c["covis_weight"][k])) for k in range(c["covis_start"][i], c["covis_start"][i + 1]) if c["covis"][k] != 5]
            if i != 5 else [] for i in range(n)]
    c["covis_start"], flat = _csr(keep)
    c["covis"], c["covis_weight"] = np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.int32)
    return c


def _two_loops():
    n = 16
    loop_edges = [[] for _ in range(n)]
    loop_edges[12], loop_edges[3] = [3], [12]
    return build(n, 23, loop_edges=loop_edges, loop_conn=[(15, 0, 60), (14, 1, 140)])


BUILDERS = {
    "two": lambda: build(2, 40, covis_back=0, corrected=(-1,)),
    "chain3": lambda: build(3, 32, covis_back=0, loop_conn=[(2, 0, 150)], corrected=(-1,)),
    "ring12": lambda: build(12, 13),
    "ring12_fix_scale": lambda: build(12, 30, fix_scale=1, iterations=3),
    "ring12_bad_middle": lambda: build(12, 14, kf_bad=(6,)),
    "ring12_bad_loop_kf": lambda: build(12, 30, kf_bad=(0,), loop_conn=[(11, 0, 60), (11, 1, 130)], iterations=1),
    "isolated": _isolated,
    "filters": _filters,
    "kf40": lambda: build(40, 16, covis_back=8, loop_conn=[(39, 0, 60), (39, 1, 105), (38, 0, 110)]),
    "two_loops": _two_loops,
    # seventy rows reach column 1: more than the 64 panel blocks k_eg_step keeps in LDS
    "hub80": lambda: build(80, 24, loop_edges=[[1] if i >= 10 else [] for i in range(80)], iterations=1),
    "consistent": lambda: build(12, 36, no_maps=True),
    "drift_known": lambda: build(12, 30, all_maps=True, xi_scale=0.5, iterations=4),
    "drift_known_fix_scale": lambda: build(12, 30, all_maps=True, xi_scale=0.5, fix_scale=1, iterations=4),
    "nothing": lambda: build(2, 19, covis_back=0, loop_conn=np.zeros((0, 3), np.int32), parent=[-1, -1], no_maps=True),
}
# THE ITERATION LIMITS.  Levenberg's last iterations run at the noise floor of the numeric Jacobian (rounding divided by 1e-9): whether
# a step that changes chi2 by 1e-17 is accepted depends on the arithmetic form, and with it the number of iterations and trials.  A
# case whose run ends there is kept only with a seed at which all forms of the reference agree on every integer
# (test_integers_agree_under_every_form); the others end by their iteration limit while every step is still accepted decisively.
NAMES = tuple(BUILDERS)
_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


_REF = {}


def reference(name, form=ER.DEVICE_FORM, rules=ER.REFERENCE):
    """The reference's result of a case under one form, computed once and shared."""
    key = (name, form, rules)
    if key not in _REF:
        _REF[key] = ER.optimize_essential_graph(case(name), form, rules)
    return _REF[key]


def ulps(a, b, dtype):
    """|a - b| in units in the last place of the larger magnitude (at least the smallest normal)."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    fi = np.finfo(dtype)
    scale = np.maximum(np.maximum(np.abs(a), np.abs(b)), fi.tiny)
    return np.abs(a - b) / (2.0 ** np.floor(np.log2(scale)) * fi.eps)


def measure_spread(name):
    """The largest difference, in ulps of its format, between the device form and every other form of the reference, per output."""
    base = dict(reference(name))
    base["rel"] = relative(base["sim3"], base["edges"])
    out = {k: 0.0 for k in FLOAT_OUTPUTS + DOUBLE_OUTPUTS}
    ints = True
    for form in ER.FORMS[1:]:
        r = dict(reference(name, form))
        r["rel"] = relative(r["sim3"], r["edges"])
        ints = ints and all(r[k] == base[k] for k in ("status", "ret", "iterations", "trials", "edges"))
        for k in FLOAT_OUTPUTS:
            out[k] = max(out[k], float(ulps(base[k], r[k], f32).max()) if np.size(base[k]) else 0.0)
        for k in DOUBLE_OUTPUTS:
            out[k] = max(out[k], float(chi_ulps(base[k], r[k]).max()) if np.size(base[k]) else 0.0)
    out["integers_agree"] = bool(ints)
    return out


def chi_ulps(a, b):
    """Double ulps.  An entry that is small against the largest of its kind -- of its column for the [n][8] Sim3 arrays (a quaternion
    component, a translation component, the scale), of the whole array for the edges' chi2 -- is measured at 2^-20 of that largest
    value: a quaternion or translation component near zero is a sum of products of its column's magnitude, so its rounding is absolute
    at that magnitude however small the sum comes out, and an edge's chi2 at the optimum is a difference of roundings."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    if not a.size:
        return np.zeros(a.shape, f64)
    m = np.maximum(np.abs(a), np.abs(b))
    top = m.max(0, keepdims=True) if a.ndim == 2 else m.max()
    scale = np.maximum(np.maximum(m, top * 2.0 ** -20), np.finfo(f64).tiny)
    return np.abs(a - b) / (2.0 ** np.floor(np.log2(scale)) * np.finfo(f64).eps)


def relative(sim3, edges):
    """Per edge (i, j, kind) the Sim3 S_j * S_i^-1 of the recovered estimates [n][8] as [edges][8]: what a common transform of the
    world leaves alone, so the one output of the graph without a gauge (a bad loop_kf) that its missing gauge does not move."""
    sim3 = np.asarray(sim3, f64).reshape(-1, 8)
    out = np.zeros((len(edges), 8), f64)
    for k, e in enumerate(edges):
        Si, Sj = (Sim3(sim3[v, :4], sim3[v, 4:7], sim3[v, 7]) for v in (int(e[0]), int(e[1])))
        with np.errstate(all="ignore"):
            S = sim3_mul(Sj, sim3_inverse(Si))
        out[k] = np.concatenate([S.q, S.t, [S.s]])
    return out


def load_spread():
    with open(SPREAD_PATH) as f:
        return json.load(f)


def bounds(name):
    """Per output the larger of 2 ulps of its format and 16 x the recorded spread of the case."""
    s = load_spread()[name]
    return {k: max(2.0, 16.0 * s[k]) for k in FLOAT_OUTPUTS + DOUBLE_OUTPUTS}


def compare(name, got, ref=None):
    """got: dict with status, ret, iterations, trials, free, vertices, kinds, edges [(i, j, kind)], Tcw, Ow, pos, sim3, chi2.  Returns the
    list of failures (empty = within the bounds) and the measured ulps per output."""
    ref = dict(reference(name) if ref is None else ref)
    got = dict(got)
    for r in (ref, got):
        if "rel" not in r:
            r["rel"] = relative(r["sim3"], r["edges"])
    bad, seen = [], {}
    for k in ("status", "ret", "iterations", "trials", "free", "vertices", "kinds"):
        if got[k] != ref[k]:
            bad.append("%s: %r != %r" % (k, got[k], ref[k]))
    if [tuple(int(x) for x in e) for e in got["edges"]] != [tuple(e) for e in ref["edges"]]:
        bad.append("the edge lists differ")
    bd = bounds(name)
    for k in FLOAT_OUTPUTS + DOUBLE_OUTPUTS:
        a, b = np.asarray(got[k], f64), np.asarray(ref[k], f64)
        if a.shape != b.shape:
            bad.append("%s: shape %s != %s" % (k, a.shape, b.shape))
            continue
        if not a.size:
            seen[k] = 0.0
            continue
        u = ulps(a, b, f32) if k in FLOAT_OUTPUTS else chi_ulps(a, b)
        seen[k] = float(u.max())
        if not np.isfinite(a).all() or seen[k] > bd[k]:
            bad.append("%s: %.3g ulps > %.3g" % (k, seen[k], bd[k]))
    return bad, seen
