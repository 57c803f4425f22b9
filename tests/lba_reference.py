"""Optimizer::LocalBundleAdjustment (thirdparty/orb-slam2/src/Optimizer.cc:453-778, monocular) and the g2o path under it as a plain
dense numpy-float64 restatement -- the reference of tests/test_local_bundle_adjustment.py for pilotguru_amd/csrc/local_ba.hip.
A helper module (no tests).

It restates: the set derivation of :455-504 as flags, VertexSE3Expmap / VertexSBAPointXYZ (oplus), EdgeSE3ProjectXYZ (computeError,
the analytic linearizeOplus, types_six_dof_expmap.cpp:103-139), RobustKernelHuber, BaseBinaryEdge::constructQuadraticForm,
BlockSolver_6_3::solve (block_solver.hpp:353-486: Eigen's 3 x 3 cofactor inverse, the Schur complement, the landmark
back-substitution), a dense Cholesky for LinearSolverEigen, OptimizationAlgorithmLevenberg::solve and the two classifications.
The SE3Quat pieces are those of tests/pose_reference.py.

UNPINNED: g2o and Eigen cannot be built where this suite runs.  The readings are the ten of DESIGN.md section 5; `Rules` switches each
to its mutant, `Form` switches the arithmetic forms whose spread sets the tolerances: contraction of a*b + c to one rounding
(emulated in long double), the order of the sums (table order, a permuted order standing in for g2o's id / insertion order, the
device's reduction tree for chi2 and computeScale), and the Cholesky as LLT or LDLT.

Non-finite rule (the library implements the same): when the active chi2 a Levenberg iteration starts from is not finite, or an
edge's chi2 at a classification is not, the window ends with every output as the input, the per-observation outputs 0, LBA_NONFINITE."""
from dataclasses import dataclass, replace

import numpy as np

import pose_reference as PR

f32, f64, ld = np.float32, np.float64, np.longdouble
LBA_NOTHING, LBA_NONFINITE = 1, 2
INFO = 10
ROLE_NONE, ROLE_LOCAL, ROLE_FIXED = 0, 1, 2
DELTA = PR.DELTA
DBL_MAX = PR.DBL_MAX
CHI2 = 5.991
MAX_LOCAL_KF, MAX_FIXED_KF, MAX_POINTS, MAX_EDGES = 64, 256, 8192, 65536


@dataclass(frozen=True)
class Rules:
    lambda_reset: bool = True          # iteration 0 of each optimize() call runs computeLambdaInit (reading 5)
    lambda_on_hll: bool = True         # setLambda adds to the landmark diagonals too (reading 5)
    lambda_init_points: bool = True    # computeLambdaInit runs over every active vertex (reading 5)
    fixed_hpp: bool = False            # a fixed camera gets a pose block (reading 3; mutant)
    huber_round2: bool = False         # setRobustKernel(0) before the second optimize (:685)
    stale_errors: bool = True          # no computeError after a rejected trial (reading 6)
    stale_level1: bool = True          # a level-1 edge keeps its round-1 chi2 (reading 7)
    stale_depth: bool = False          # a level-1 edge's isDepthPositive where its error was computed, not at the final estimates (mutant)
    drop_inactive: bool = True         # initializeOptimization drops vertices without a level-0 edge (reading 8)
    stop_rule: bool = True             # (iniChi-currentChi)*1e3<iniChi three times running
    fix_id0: bool = True               # setFixed(pKFi->mnId==0) (:529)
    skip_bad_kf_obs: bool = True       # if(!pKFi->isBad()) at the edges (:589)


REFERENCE = Rules()
MUTANTS = {
    "lambda_without_round_reset": replace(REFERENCE, lambda_reset=False),
    "lambda_not_on_hll": replace(REFERENCE, lambda_on_hll=False),
    "lambda_init_over_poses_only": replace(REFERENCE, lambda_init_points=False),
    "fixed_camera_gets_hpp": replace(REFERENCE, fixed_hpp=True),
    "huber_kept_in_round2": replace(REFERENCE, huber_round2=True),
    "errors_recomputed_after_reject": replace(REFERENCE, stale_errors=False),
    "level1_chi2_recomputed": replace(REFERENCE, stale_level1=False),
    "depth_on_stale_estimates": replace(REFERENCE, stale_depth=True),
    "inactive_vertex_kept": replace(REFERENCE, drop_inactive=False),
    "no_1e3_stop_rule": replace(REFERENCE, stop_rule=False),
    "id0_not_fixed": replace(REFERENCE, fix_id0=False),
    "bad_kf_observations_kept": replace(REFERENCE, skip_bad_kf_obs=False),
}


@dataclass(frozen=True)
class Form:
    fma: bool = False
    order: str = "table"               # "table" | "perm" | "tree"
    chol: str = "llt"                  # "llt" | "ldlt"


FORMS = [Form(fma, order, chol) for fma in (False, True) for order in ("table", "perm", "tree") for chol in ("llt", "ldlt")]


class Problem:
    """One window over a batch's frames and the resident table, as the interface takes it.  keys_xy[f] float32 [n][2], octaves[f],
    pose dicts {Tcw [12], fx, fy, cx, cy} per frame, kf_bad [nf], kf_point[f] [n] (table index or -1), fixed_id0 [nf], local_kf (frame
    indices), pos float32 [np][3], point_bad [np], the CSR obs_start / obs_frame / obs_idx, inv_sigma2 (float, by octave)."""

    def __init__(self, keys_xy, octaves, Tcw, cam, kf_bad, kf_point, fixed_id0, local_kf, pos, point_bad, obs_start, obs_frame, obs_idx,
                 inv_sigma2=None, name=""):
        self.keys_xy = [np.asarray(k, f32).reshape(-1, 2) for k in keys_xy]
        self.octaves = [np.asarray(o, np.int32) for o in octaves]
        self.Tcw = np.asarray(Tcw, f32).reshape(-1, 12)
        self.cam = np.asarray(cam, f32).reshape(-1, 4)
        self.kf_bad = np.asarray(kf_bad, np.uint8)
        self.kf_point = [np.asarray(s, np.int32) for s in kf_point]
        self.fixed_id0 = np.asarray(fixed_id0, np.uint8)
        self.local_kf = np.asarray(local_kf, np.int32)
        self.pos = np.asarray(pos, f32).reshape(-1, 3)
        self.point_bad = np.asarray(point_bad, np.uint8)
        self.obs_start, self.obs_frame, self.obs_idx = (np.asarray(a, np.int32) for a in (obs_start, obs_frame, obs_idx))
        self.inv_sigma2 = PR.inv_level_sigma2() if inv_sigma2 is None else np.asarray(inv_sigma2, f32)
        self.name = name

    @property
    def nframes(self):
        return len(self.keys_xy)


# ---------------------------------------------------------------- the sets (:455-504) as flags
def derive_sets(P, rules=REFERENCE):
    """(is_local [np], role [nf], edge [nobs]): local points = not bad, in a slot of a local key frame that is not bad; fixed = not
    bad, observes a local point, not local; edges = the observations of local points in frames that are not bad."""
    nf, npts = P.nframes, len(P.pos)
    role = np.zeros(nf, np.uint8)
    for f in P.local_kf:
        if not P.kf_bad[f]:
            role[f] = ROLE_LOCAL
    is_local = np.zeros(npts, np.uint8)
    for f in range(nf):
        if role[f] == ROLE_LOCAL:
            s = P.kf_point[f]
            s = s[(s >= 0) & (s < npts)]
            is_local[s[P.point_bad[s] == 0]] = 1
    pt_of = np.repeat(np.arange(npts), np.diff(P.obs_start))
    in_local = is_local[pt_of] == 1
    listed = np.zeros(nf, bool)
    listed[P.local_kf] = True            # mnBALocalForKF is set for a bad neighbour too (:465): it can never become fixed
    for f in np.unique(P.obs_frame[in_local]):
        if not listed[f] and not P.kf_bad[f]:
            role[f] = ROLE_FIXED
    edge = in_local & ((P.kf_bad[P.obs_frame] == 0) if rules.skip_bad_kf_obs else True)
    return is_local, role, edge.astype(np.uint8)


def literal_sets(P):
    """Optimizer.cc:455-504 transcribed with its lists and marks; returns (set of local points, set of fixed frames, set of (point, frame)
    edges).  pKF is local_kf[0], the neighbours follow."""
    mark_local_kf, mark_fixed_kf, mark_pt = set(), set(), set()
    lLocalKeyFrames = [int(P.local_kf[0])]
    mark_local_kf.add(int(P.local_kf[0]))
    for f in P.local_kf[1:]:
        mark_local_kf.add(int(f))
        if not P.kf_bad[f]:
            lLocalKeyFrames.append(int(f))
    lLocalMapPoints = []
    for f in lLocalKeyFrames:
        for s in P.kf_point[f]:
            if s >= 0 and not P.point_bad[s] and s not in mark_pt:
                lLocalMapPoints.append(int(s))
                mark_pt.add(int(s))
    lFixedCameras = []
    for p in lLocalMapPoints:
        for k in range(P.obs_start[p], P.obs_start[p + 1]):
            f = int(P.obs_frame[k])
            if f not in mark_local_kf and f not in mark_fixed_kf:
                mark_fixed_kf.add(f)
                if not P.kf_bad[f]:
                    lFixedCameras.append(f)
    edges = set()
    for p in lLocalMapPoints:
        for k in range(P.obs_start[p], P.obs_start[p + 1]):
            if not P.kf_bad[P.obs_frame[k]]:
                edges.add((p, int(P.obs_frame[k])))
    return set(lLocalKeyFrames), set(lLocalMapPoints), set(lFixedCameras), edges


# ---------------------------------------------------------------- arithmetic forms
def fmadd(a, b, c, form):
    """a*b + c: two roundings, or (contracted) one, emulated in long double."""
    if form.fma:
        return (np.asarray(a, ld) * np.asarray(b, ld) + np.asarray(c, ld)).astype(f64)
    return a * b + c


def tree_sum(*lists):
    """The device's chi2 / scale reduction: item i of each list belongs to thread i mod 256, which sums its items list after list and
    in order; a xor butterfly inside each 64-lane wave, then (w0 + w1) + (w2 + w3)."""
    part = np.zeros(256, f64)
    for v in lists:
        v = np.asarray(v, f64)
        for i0 in range(0, len(v), 256):
            c = v[i0:i0 + 256]
            part[:len(c)] = part[:len(c)] + c
    idx = np.arange(256)
    for m in (32, 16, 8, 4, 2, 1):
        part = part + part[idx ^ m]
    return (part[0] + part[64]) + (part[128] + part[192])


def seq_sum(v):
    v = np.asarray(v, f64)
    return np.add.accumulate(v)[-1] if len(v) else f64(0.0)


# ---------------------------------------------------------------- the edge
class Graph:
    pass


def build_graph(P, is_local, role, edge, rules, form):
    G = Graph()
    pts = np.flatnonzero(is_local)
    comp = -np.ones(len(P.pos), np.int64)
    comp[pts] = np.arange(len(pts))
    pt_of = np.repeat(np.arange(len(P.pos)), np.diff(P.obs_start))
    ks = np.flatnonzero(edge)
    if form.order == "perm":               # another point order and another order inside each list: g2o's id / insertion order
        rng = np.random.default_rng(12345)
        key = rng.permutation(len(P.pos))[pt_of[ks]].astype(f64) + rng.random(len(ks)) * 0.5
        ks = ks[np.argsort(key, kind="stable")]
    G.k = ks
    G.pt = comp[pt_of[ks]]
    G.frame = P.obs_frame[ks].astype(np.int64)
    G.obs = np.stack([P.keys_xy[f][i] for f, i in zip(G.frame, P.obs_idx[ks])]).astype(f64).reshape(-1, 2) if len(ks) else np.zeros((0, 2))
    G.w = np.array([P.inv_sigma2[P.octaves[f][i]] for f, i in zip(G.frame, P.obs_idx[ks])], f32).astype(f64)
    G.pts = pts
    fixed = np.ones(P.nframes, bool)
    for f in range(P.nframes):
        if role[f] == ROLE_LOCAL and not (rules.fix_id0 and P.fixed_id0[f]):
            fixed[f] = False
    if rules.fixed_hpp:
        fixed[role == ROLE_FIXED] = False
    G.free = np.flatnonzero(~fixed)
    G.col = -np.ones(P.nframes, np.int64)
    G.col[G.free] = np.arange(len(G.free))
    G.really_fixed = np.ones(P.nframes, bool)          # the estimates that never move, whatever block the mutant gives them
    for f in range(P.nframes):
        if role[f] == ROLE_LOCAL and not (rules.fix_id0 and P.fixed_id0[f]):
            G.really_fixed[f] = False
    G.cam = P.cam.astype(f64)
    return G


def project(q, t, X, G, sel):
    """computeError: obs - cam_project(estimate.map(point)); returns (x, y, z), e0, e1 for the edges sel."""
    f, p = G.frame[sel], G.pt[sel]
    with np.errstate(all="ignore"):
        rx, ry, rz = PR.rotate((q[f, 0], q[f, 1], q[f, 2], q[f, 3]), X[p, 0], X[p, 1], X[p, 2])
        x, y, z = rx + t[f, 0], ry + t[f, 1], rz + t[f, 2]
        e0 = G.obs[sel, 0] - ((x / z) * G.cam[f, 0] + G.cam[f, 2])
        e1 = G.obs[sel, 1] - ((y / z) * G.cam[f, 1] + G.cam[f, 3])
    return (x, y, z), e0, e1


def jacobians(q, pc, G, sel):
    """linearizeOplus (types_six_dof_expmap.cpp:103-139): Ji [m][2][3] = -1./z * tmp * R, Jj [m][2][6]."""
    f = G.frame[sel]
    fx, fy = G.cam[f, 0], G.cam[f, 1]
    x, y, z = pc
    m = len(x)
    with np.errstate(all="ignore"):
        z2 = z * z
        R = np.stack([PR.matrix_from_quat(q[a]) for a in range(len(q))])[f] if m else np.zeros((0, 3, 3))
        s = -1.0 / z
        zero = np.zeros(m)
        tmp = np.array([[s * fx, s * zero, s * (-x / z * fx)], [s * zero, s * fy, s * (-y / z * fy)]])      # [2][3][m]
        Ji = np.zeros((m, 2, 3))
        for r in range(2):
            for c in range(3):
                Ji[:, r, c] = (tmp[r, 0] * R[:, 0, c] + tmp[r, 1] * R[:, 1, c]) + tmp[r, 2] * R[:, 2, c]
        Jj = np.zeros((m, 2, 6))
        Jj[:, 0] = np.stack([x * y / z2 * fx, -(1.0 + (x * x / z2)) * fx, y / z * fx, -1.0 / z * fx, zero, x / z2 * fx], 1)
        Jj[:, 1] = np.stack([(1.0 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, zero, -1.0 / z * fy, y / z2 * fy], 1)
    return Ji, Jj


def atb(A, wO, B, form):
    """A' * (wO * I) * B per edge: [m][a][b] = (A[0][a]*wO)*B[0][b] + (A[1][a]*wO)*B[1][b]."""
    s0 = (A[:, 0, :] * wO[:, None])[:, :, None]
    s1 = (A[:, 1, :] * wO[:, None])[:, :, None]
    return fmadd(s1, B[:, 1, None, :], s0 * B[:, 0, None, :], form)


def inverse3(D):
    """Eigen's fixed-size 3 x 3 inverse: cofactors, det = the first cofactor column times the first matrix column, no test."""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return D[i1, j1] * D[i2, j2] - D[i1, j2] * D[i2, j1]
    with np.errstate(all="ignore"):
        c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
        det = (c0[0] * D[0, 0] + c0[1] * D[1, 0]) + c0[2] * D[2, 0]
        inv = 1.0 / det
        out = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                out[j, i] = (c0[i] if j == 0 else cof(i, j)) * inv
        return out


def cholesky_solve(A, b, form, margins):
    """The dense Cholesky of the reduced system, right-looking in index order; (ok, x).  ok = every pivot positive."""
    n = len(b)
    A = A.copy()
    y = b.copy()
    ok = True
    if n == 0:
        return True, y
    scale = max(np.max(np.abs(np.diag(A))), 1e-300)
    with np.errstate(all="ignore"):
        if form.chol == "llt":
            for k in range(n):
                d = A[k, k]
                margins["pivot"] = min(margins.get("pivot", np.inf), abs(d) / scale)
                ok = ok and bool(d > 0)
                A[k, k] = np.sqrt(d)
                A[k + 1:, k] = A[k + 1:, k] / A[k, k]
                c = A[k + 1:, k]
                A[k + 1:, k + 1:] = fmadd(-c[:, None], c[None, :], A[k + 1:, k + 1:], form)
            for k in range(n):
                y[k] = y[k] / A[k, k]
                y[k + 1:] = fmadd(-A[k + 1:, k], y[k], y[k + 1:], form)
            for k in range(n - 1, -1, -1):
                y[k] = y[k] / A[k, k]
                y[:k] = fmadd(-A[k, :k], y[k], y[:k], form)
        else:
            for k in range(n):
                d = A[k, k]
                margins["pivot"] = min(margins.get("pivot", np.inf), abs(d) / scale)
                ok = ok and bool(d > 0)
                c = A[k + 1:, k].copy()
                A[k + 1:, k] = c / d
                A[k + 1:, k + 1:] = fmadd(-A[k + 1:, k, None], c[None, :], A[k + 1:, k + 1:], form)
            for k in range(n):
                y[k + 1:] = fmadd(-A[k + 1:, k], y[k], y[k + 1:], form)
            y = y / np.diag(A)
            for k in range(n - 1, -1, -1):
                y[:k] = fmadd(-A[k, :k], y[k], y[:k], form)
    return ok, y


class State:
    pass


def linear_system(S, G, act, robust, form):
    """computeActiveErrors, activeRobustChi2 and buildSystem over the level-0 edges `act` (indices into G)."""
    pc, e0, e1 = project(S.q, S.t, S.X, G, act)
    S.err[act, 0], S.err[act, 1] = e0, e1
    w = G.w[act]
    c2 = PR.edge_chi2(e0, e1, w)
    rho0, rho1 = PR.huber(c2) if robust else (c2, np.ones_like(c2))
    Ji, Jj = jacobians(S.q, pc, G, act)
    wO = rho1 * w
    with np.errstate(all="ignore"):
        r0, r1 = -(w * e0) * rho1, -(w * e1) * rho1              # omega_r = -omega * _error, then *= rho[1]
    ncam, npt = len(G.free), len(G.pts)
    col, p = G.col[G.frame[act]], G.pt[act]
    Hll = np.zeros((npt, 3, 3))
    bl = np.zeros((npt, 3))
    np.add.at(Hll, p, atb(Ji, wO, Ji, form))
    np.add.at(bl, p, fmadd(Ji[:, 1, :], r1[:, None], Ji[:, 0, :] * r0[:, None], form))
    Hpp = np.zeros((ncam, 6, 6))
    bp = np.zeros((ncam, 6))
    fr = col >= 0
    np.add.at(Hpp, col[fr], atb(Jj, wO, Jj, form)[fr])
    np.add.at(bp, col[fr], fmadd(Jj[:, 1, :], r1[:, None], Jj[:, 0, :] * r0[:, None], form)[fr])
    W = atb(Jj, wO, Ji, form)                                   # the pose-landmark blocks [m][6][3]
    return rho0, Hpp, bp, Hll, bl, W, col, p


def chi2_sum(rho0, p, npt, form):
    """activeRobustChi2: edge by edge; the device sums each point's edges, then the points in its tree."""
    if form.order == "tree":
        per = np.zeros(npt)
        np.add.at(per, p, rho0)
        return tree_sum(per)
    return seq_sum(rho0)


def schur_solve(Hpp, bp, Hll, bl, W, col, p, lam, lam_l, act_cam, act_pt, form, margins):
    """BlockSolver::solve with lambda on the diagonals; (ok, xp [ncam][6], xl [npt][3])."""
    ncam, npt = len(Hpp), len(Hll)
    n = 6 * ncam
    Hs = np.zeros((n, n))
    for c in range(ncam):
        Hs[6 * c:6 * c + 6, 6 * c:6 * c + 6] = Hpp[c] + (np.eye(6) * lam if act_cam[c] else 0.0)
    coef = np.zeros(n)
    Dinv = np.zeros((npt, 3, 3))
    fr = np.flatnonzero(col >= 0)
    order = np.argsort(p[fr], kind="stable")
    fr = fr[order]
    starts = np.searchsorted(p[fr], np.arange(npt + 1))
    with np.errstate(all="ignore"):
        for j in range(npt):
            if not act_pt[j]:
                continue
            Dinv[j] = inverse3(Hll[j] + np.eye(3) * lam_l)
            es = fr[starts[j]:starts[j + 1]]
            if not len(es):
                continue
            Wj = np.zeros((n, 3))
            for e in es:
                Wj[6 * col[e]:6 * col[e] + 6] = W[e]
            db = Dinv[j] @ bl[j]
            BD = Wj @ Dinv[j]
            coef = coef + Wj @ db
            Hs = fmadd(-BD[:, None, 0], Wj[None, :, 0], Hs, form)
            Hs = fmadd(-BD[:, None, 1], Wj[None, :, 1], Hs, form)
            Hs = fmadd(-BD[:, None, 2], Wj[None, :, 2], Hs, form)
        bs = bp.reshape(-1) - coef
        keep = np.repeat(np.asarray(act_cam, bool), 6)
        A = Hs[np.ix_(keep, keep)]
        A = np.triu(A) + np.triu(A, 1).T                        # g2o fills the upper block triangle only (:419-430)
        ok, x = cholesky_solve(A, bs[keep], form, margins)
        xp = np.zeros(n)
        xp[keep] = x
        xl = np.zeros((npt, 3))
        if ok:
            cl = bl.copy()
            for e in fr:                                        # cl = bl - B' * xp, an edge at a time
                cl[p[e]] = cl[p[e]] - W[e].T @ xp[6 * col[e]:6 * col[e] + 6]
            for j in range(npt):
                if act_pt[j]:
                    xl[j] = Dinv[j] @ cl[j]
    return ok, xp.reshape(ncam, 6), xl


def optimize(S, G, level, iterations, robust, rules, form, info, margins):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg over the level-0 edges; False = not finite."""
    act = np.flatnonzero(level == 0)
    its = trials = 0
    ncam, npt = len(G.free), len(G.pts)
    if rules.drop_inactive:
        act_cam = np.zeros(ncam, bool)
        act_cam[G.col[G.frame[act]][G.col[G.frame[act]] >= 0]] = True
        act_pt = np.zeros(npt, bool)
        act_pt[G.pt[act]] = True
    else:
        act_cam, act_pt = np.ones(ncam, bool), np.ones(npt, bool)
    if len(act) == 0:
        return True, its, trials
    for it in range(iterations):
        rho0, Hpp, bp, Hll, bl, W, col, p = linear_system(S, G, act, robust, form)
        S.err_q, S.err_t, S.err_X = S.q.copy(), S.t.copy(), S.X.copy()
        current = chi2_sum(rho0, p, npt, form)
        ini = current
        if not np.isfinite(current):
            return False, its, trials
        if it == 0 and (rules.lambda_reset or S.lam is None):
            md = 0.0
            if ncam:
                md = max(md, np.max(np.abs(np.stack([np.diag(h) for h in Hpp])[act_cam]), initial=0.0))
            if rules.lambda_init_points and npt:
                md = max(md, np.max(np.abs(np.stack([np.diag(h) for h in Hll])[act_pt]), initial=0.0))
            S.lam, S.ni, S.nbad = 1e-5 * md, 2, 0
        elif it == 0:
            S.ni, S.nbad = 2, 0
        its += 1
        rho, qmax = 0.0, 0
        while True:
            ok, xp, xl = schur_solve(Hpp, bp, Hll, bl, W, col, p, S.lam, S.lam if rules.lambda_on_hll else 0.0, act_cam, act_pt, form, margins)
            q2, t2, X2 = S.q.copy(), S.t.copy(), S.X.copy()
            if ok:
                for c, f in enumerate(G.free):
                    if act_cam[c] and not G.really_fixed[f]:
                        E = PR.oplus(PR.SE3(S.q[f], S.t[f]), xp[c])
                        q2[f], t2[f] = E.q, E.t
                X2[act_pt] = S.X[act_pt] + xl[act_pt]
            else:
                xp, xl = np.zeros_like(xp), np.zeros_like(xl)
            _, e0, e1 = project(q2, t2, X2, G, act)
            S.err[act, 0], S.err[act, 1] = e0, e1
            S.err_q, S.err_t, S.err_X = q2, t2, X2
            c2 = PR.edge_chi2(e0, e1, G.w[act])
            temp = chi2_sum(PR.huber(c2)[0] if robust else c2, p, npt, form)
            if not ok:
                temp = DBL_MAX
            with np.errstate(all="ignore"):
                tp, tl = (xp * (S.lam * xp + bp)).reshape(-1), xl * (S.lam * xl + bl)
                if form.order == "tree":                        # the device: the camera rows, then each point's (t0 + t1) + t2
                    scale = tree_sum(tp, (tl[:, 0] + tl[:, 1]) + tl[:, 2]) + 1e-3
                else:                                           # computeScale: every dimension in turn, poses first
                    scale = seq_sum(np.concatenate([tp, tl.reshape(-1)])) + 1e-3
                rho = (current - temp) / scale
            if ok:
                margins["rho"] = min(margins.get("rho", np.inf), abs(rho)) if rho != 0.0 else margins.get("rho", np.inf)
            if rho > 0 and np.isfinite(temp):
                tt = 2.0 * rho - 1.0
                alpha = min(1.0 - (tt * tt) * tt, 2.0 / 3.0)
                S.lam *= max(1.0 / 3.0, alpha)
                S.ni = 2
                current = temp
                S.q, S.t, S.X = q2, t2, X2
                S.last_rejected = False
            else:
                S.lam *= S.ni
                S.ni *= 2
                S.last_rejected = True
                if not rules.stale_errors:
                    _, e0, e1 = project(S.q, S.t, S.X, G, act)
                    S.err[act, 0], S.err[act, 1] = e0, e1
                    S.err_q, S.err_t, S.err_X = S.q.copy(), S.t.copy(), S.X.copy()
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            info["terminate"] = info.get("terminate", 0) + 1
            break
        if ini > 0:
            margins["stop"] = min(margins.get("stop", np.inf), abs((ini - current) * 1e3 - ini) / ini)
        if rules.stop_rule:
            S.nbad = S.nbad + 1 if (ini - current) * 1e3 < ini else 0
            if S.nbad >= 3:
                info["stopped_by_1e3"] = info.get("stopped_by_1e3", 0) + 1
                break
    return True, its, trials


def classify(S, G, sel, rules, margins, level=None, round1=None):
    """e->chi2() > 5.991 || !e->isDepthPositive() for the edges sel: chi2 of the stored errors, depth of the estimates.  The mutant
    reads a level-1 edge's depth where its stored error was computed: at the end of the first optimize."""
    c2 = PR.edge_chi2(S.err[sel, 0], S.err[sel, 1], G.w[sel])
    pc, _, _ = project(S.q, S.t, S.X, G, sel)
    z = pc[2]
    if rules.stale_depth and round1 is not None:
        z = np.where(level[sel] == 1, project(round1[0], round1[1], round1[2], G, sel)[0][2], z)
    if len(sel):
        with np.errstate(all="ignore"):
            margins["chi2"] = min(margins.get("chi2", np.inf), float(np.min(np.abs(c2 - CHI2) / CHI2)))
            margins["depth"] = min(margins.get("depth", np.inf), float(np.min(np.abs(z))))
    return c2, (c2 > CHI2) | ~(z > 0.0)


def local_bundle_adjustment(P, rounds=2, rules=REFERENCE, form=Form()):
    """Returns a dict: ret, pose_Tcw [nf][12] / pose_Ow [nf][3] (float, local key frames; the input elsewhere), pos [np][3] float,
    erase / chi2 / level [nobs], is_local, role, info [INFO], and `margins` and `hits` for the case condition."""
    nobs = len(P.obs_frame)
    is_local, role, edge = derive_sets(P, rules)
    G = build_graph(P, is_local, role, edge, rules, form)
    ne = len(G.k)
    out = dict(ret=0, pos=P.pos.copy(), erase=np.zeros(nobs, np.uint8), chi2=np.zeros(nobs, f32), level=np.zeros(nobs, np.uint8),
               is_local=is_local, role=role, info=np.zeros(INFO, np.int32), margins={}, hits={})
    out["pose_Tcw"], out["pose_Ow"] = P.Tcw.copy(), None      # pose_Ow None: pose_out is the input record byte for byte
    info = out["info"]
    info[1:5] = ne, len(G.pts), int(np.sum(role == ROLE_LOCAL)), int(np.sum(role == ROLE_FIXED))
    if ne == 0:
        info[0] = LBA_NOTHING
        return out
    S = State()
    S.q = np.zeros((P.nframes, 4))
    S.t = np.zeros((P.nframes, 3))
    for f in range(P.nframes):
        if role[f]:
            E = PR.to_se3(P.Tcw[f])
            S.q[f], S.t[f] = E.q, E.t
        else:
            S.q[f] = (0, 0, 0, 1)
    S.X = P.pos[G.pts].astype(f64)
    S.err = np.zeros((ne, 2))
    S.err_q, S.err_t, S.err_X = S.q.copy(), S.t.copy(), S.X.copy()
    S.lam, S.ni, S.nbad, S.last_rejected = None, 2, 0, False
    level = np.zeros(ne, np.int64)
    hits, margins = out["hits"], out["margins"]
    fine, info[5], info[6] = optimize(S, G, level, 5, True, rules, form, hits, margins)
    hits["round1_ended_rejected"] = int(S.last_rejected)
    everything = np.arange(ne)
    round1 = None
    if fine and rounds >= 2:
        round1 = (S.q.copy(), S.t.copy(), S.X.copy())
        c2, bad = classify(S, G, everything, rules, margins)
        fine = bool(np.all(np.isfinite(c2)))
        level[bad] = 1
        info[9] = int(np.sum(bad))
        hits["set_aside_for_depth_alone"] = int(np.sum(bad & (c2 <= CHI2)))
        if fine:
            fine, info[7], info[8] = optimize(S, G, level, 10, rules.huber_round2, rules, form, hits, margins)
    if fine:
        if not rules.stale_level1:
            l1 = np.flatnonzero(level == 1)
            _, e0, e1 = project(S.q, S.t, S.X, G, l1)
            S.err[l1, 0], S.err[l1, 1] = e0, e1
        c2, bad = classify(S, G, everything, rules, margins, level, round1)
        fine = bool(np.all(np.isfinite(c2)))
    if not fine:
        info[0] = LBA_NONFINITE
        info[5:10] = 0
        return out
    out["erase"][G.k] = bad
    out["chi2"][G.k] = c2.astype(f32)
    out["level"][G.k] = level
    hits["depth_only_survivor"] = int(np.sum((level == 1) & ~bad))
    out["ret"] = int(np.sum(bad))
    out["pos"][G.pts] = S.X.astype(f32)
    out["pose_Ow"] = np.zeros((P.nframes, 3), f32)
    for f in range(P.nframes):
        if role[f] == ROLE_LOCAL:
            out["pose_Tcw"][f], out["pose_Ow"][f] = PR.to_pose_floats(PR.SE3(S.q[f], S.t[f]))
    out["estimates"] = (S.q, S.t, S.X)
    return out
