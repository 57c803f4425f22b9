"""Optimizer::OptimizeSim3 (thirdparty/orb-slam2/src/Optimizer.cc:1046-1241) and the g2o path under it as a plain sequential
numpy-float64 restatement -- the reference of tests/test_optimize_sim3.py for pilotguru_amd/csrc/optimize_sim3.hip.  A helper
module (no tests).

It restates, in the sources' operation order per edge: g2o::Sim3 (Sim3(Vector7d) with its four branches, map, inverse, operator*;
types/sim3.h), VertexSim3Expmap::oplusImpl, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError
(types_seven_dof_expmap.h), BaseBinaryEdge::linearizeOplus (the NUMERIC Jacobian: central differences through oplus with
delta = 1e-9; base_binary_edge.hpp:131-205) and constructQuadraticForm, RobustKernelHuber::robustify,
OptimizationAlgorithmLevenberg::solve, LinearSolverDense::solve, and the caller's gScm / gScm*gSmw / toCvMat steps
(LoopClosing.cc:320-335).

UNPINNED: g2o and Eigen cannot be built where this suite runs.  The readings of Eigen are those of tests/pose_reference.py (its
quaternion helpers are imported), plus: Sim3's quaternion is never renormalised; s*(r*xyz) + t is (s*rx) + tx per component;
A*Omega + B*Omega2 + C*I is (A*Om + B*Om2) + C*I per entry.  What anchors it is tested on the CPU: noise-free scenes return the
generating Sim3, the numeric Jacobian against an analytic one, the solve against numpy.linalg.solve.

ARITHMETIC FORMS.  The sums over edges go through `order` (pose_reference.osum: "edges" = e12_0, e21_0, e12_1, ... as g2o's
active edges are ordered, "reversed", "pairwise"; and "device", the kernel's own fixed tree, so that the case condition below
also covers the order the library sums in).  The fourth form, "ulp", sums like "edges" and moves every exp, sin and cos
result one ulp up (acos, the fourth libm call of sim3.h, is only in Sim3::log, which OptimizeSim3 never reaches): the device's
libm is not glibc's, and the 1e-9 differences of the Jacobian amplify exactly that.  A result at argument 0 is left alone: it is
exact in every libm.

Non-finite rule (the reference's behaviour is undefined there; the library implements the same): when the active chi2 a Levenberg
iteration starts from, or an edge's chi2 at a classification, is not finite, the result is the input estimate, the merged
matches with nothing removed, every chi2 0, 0 inliers and OS3_NONFINITE."""
import os
import sys
from dataclasses import dataclass, replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pose_reference import inv_level_sigma2, matrix_from_quat, osum, quat_from_matrix, quat_mul, rotate  # noqa: E402
from sim3_reference import gemm_rows, pose_parts  # noqa: E402

f32, f64 = np.float32, np.float64
OS3_FEW, OS3_NONFINITE = 1, 2
DBL_MAX = np.finfo(np.float64).max
FORMS = ("edges", "reversed", "pairwise", "ulp", "device")
DELTA_NUM = 1e-9


@dataclass(frozen=True)
class Rules:
    jacobian: str = "numeric"          # both linearizeOplus overrides are commented out | "analytic"
    stale_read: bool = True            # e->chi2() without computeError: the errors of the last trial (:1193, :1227)
    zero_x6: bool = True               # oplusImpl zeroes update[6] inside the solver's x before computeScale
    lambda_reset: bool = True          # computeLambdaInit at iteration 0 of each optimize() call
    more_iterations: tuple = (10, 5)   # nBad > 0: 10, else 5 (:1205-1209)
    remove_ge: bool = False            # chi2 > th2 (:1193)
    few_le: bool = False               # nCorrespondences - nBad < 10 (:1211)
    write_on_few: bool = False         # return 0 before the vertex is recovered
    huber_second: bool = True          # the kernels stay on the edges for the second optimize()
    edge_order: str = "interleaved"    # e12_0, e21_0, e12_1, ... | "blocked": every e12, then every e21
    use_new_matches: bool = True       # SearchBySim3's in-place vpMatches12[idx1] = ...


REFERENCE = Rules()
MUTANTS = {
    "analytic_jacobian": replace(REFERENCE, jacobian="analytic"),
    "errors_recomputed_before_classification": replace(REFERENCE, stale_read=False),
    "x6_not_zeroed": replace(REFERENCE, zero_x6=False),
    "lambda_carried_across_calls": replace(REFERENCE, lambda_reset=False),
    "more_iterations_swapped": replace(REFERENCE, more_iterations=(5, 10)),
    "remove_at_equal": replace(REFERENCE, remove_ge=True),
    "few_at_ten": replace(REFERENCE, few_le=True),
    "estimate_written_on_few": replace(REFERENCE, write_on_few=True),
    "huber_off_in_second_call": replace(REFERENCE, huber_second=False),
    "edge_order_blocked": replace(REFERENCE, edge_order="blocked"),
    "new_matches_ignored": replace(REFERENCE, use_new_matches=False),
}


class LibM:
    """exp, sin, cos as numpy's, or each result one ulp up (exact at 0)."""

    def __init__(self, nudge=False):
        self.nudge = nudge

    def _f(self, fn, x):
        with np.errstate(all="ignore"):
            y = f64(fn(f64(x)))
        return f64(np.nextafter(y, np.inf)) if self.nudge and x != 0 else y

    def exp(self, x):
        return self._f(np.exp, x)

    def sin(self, x):
        return self._f(np.sin, x)

    def cos(self, x):
        return self._f(np.cos, x)


def form_parts(form):
    return ("edges", LibM(True)) if form == "ulp" else (form, LibM(False))


def esum(a, order):
    """The sum of a's rows, which are e12_0, e21_0, e12_1, ...: pose_reference.osum's orders, or "device" = the kernel's fixed tree
    (correspondence k belongs to lane k mod 256, which adds its e12 row and then its e21 row in increasing k; a butterfly over
    the 64 lanes of each wave; (w0 + w1) + (w2 + w3))."""
    if order != "device":
        return osum(a, order)
    a = np.asarray(a, f64)
    m = a.shape[0] // 2
    lanes = np.zeros((256,) + a.shape[1:], f64)
    for k0 in range(0, m, 256):
        blk = a[2 * k0:2 * min(k0 + 256, m)]
        nb = blk.shape[0] // 2
        lanes[:nb] = (lanes[:nb] + blk[0::2]) + blk[1::2]
    w = lanes.reshape((4, 64) + a.shape[1:])
    for h in (32, 16, 8, 4, 2, 1):
        w = w[:, :h] + w[:, h:2 * h]
    w = w[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


# ---------------------------------------------------------------- g2o::Sim3
class Sim3:
    __slots__ = ("q", "t", "s")           # q = (x, y, z, w), never renormalised

    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.array(q, f64), np.array(t, f64), f64(s)


def _mat3(A, B):
    return np.array([[(A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c] for c in range(3)] for r in range(3)], f64)


def sim3_exp(u, lm, hits=None):
    """Sim3(Vector7d) (sim3.h:70-142); u = (omega, upsilon, sigma)."""
    u = np.asarray(u, f64)
    o0, o1, o2, sigma = u[0], u[1], u[2], u[6]
    with np.errstate(all="ignore"):
        theta = np.sqrt((o0 * o0 + o1 * o1) + o2 * o2)
        Om = np.array([[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]], f64)
        Om2 = _mat3(Om, Om)
        I = np.eye(3)
        s = lm.exp(sigma)
        eps = 0.00001
        small_theta, small_sigma = bool(theta < eps), bool(abs(sigma) < eps)
        if hits is not None:
            k = "exp_%s_sigma_%s_theta" % ("small" if small_sigma else "large", "small" if small_theta else "large")
            hits[k] = hits.get(k, 0) + 1
        if small_theta:
            R = (I + Om) + Om2
        else:
            sn, cs = lm.sin(theta), lm.cos(theta)
            R = (I + (sn / theta) * Om) + ((1.0 - cs) / (theta * theta)) * Om2
        if small_sigma:
            C = f64(1.0)
            if small_theta:
                A, B = f64(1.0) / 2.0, f64(1.0) / 6.0
            else:
                theta2 = theta * theta
                A = (1.0 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
        else:
            C = (s - 1.0) / sigma
            sigma2 = sigma * sigma
            if small_theta:
                A = ((sigma - 1.0) * s + 1.0) / sigma2
                B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
            else:
                a, b, theta2 = s * sn, s * cs, theta * theta
                c = theta2 + sigma2
                A = (a * sigma + (1.0 - b) * theta) / (theta * c)
                B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2
        W = (A * Om + B * Om2) + C * I
        t = [(W[r, 0] * u[3] + W[r, 1] * u[4]) + W[r, 2] * u[5] for r in range(3)]
    return Sim3(quat_from_matrix(R), t, s)


def sim3_mul(a, b):
    """operator*: r = a.r*b.r, t = a.s*(a.r*b.t) + a.t, s = a.s*b.s."""
    with np.errstate(all="ignore"):
        r = rotate(a.q, b.t[0], b.t[1], b.t[2])
        return Sim3(quat_mul(a.q, b.q), [a.s * r[0] + a.t[0], a.s * r[1] + a.t[1], a.s * r[2] + a.t[2]], a.s * b.s)


def sim3_inverse(a):
    """Sim3(r.conjugate(), r.conjugate()*((-1./s)*t), 1./s)."""
    with np.errstate(all="ignore"):
        k = f64(-1.0) / a.s
        q = np.array([-a.q[0], -a.q[1], -a.q[2], a.q[3]], f64)
        return Sim3(q, rotate(q, k * a.t[0], k * a.t[1], k * a.t[2]), f64(1.0) / a.s)


def oplus(est, u, fix_scale, lm, hits=None):
    """VertexSim3Expmap::oplusImpl: update[6] = 0 under _fix_scale (written into the caller's array), Sim3(update) * estimate."""
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u, lm, hits), est)


def from_estimate(R, t, s):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) of the float values."""
    return Sim3(quat_from_matrix(np.asarray(R, f32).reshape(3, 3).astype(f64)), np.asarray(t, f32).astype(f64), f64(f32(s)))


def to_estimate(S):
    return matrix_from_quat(S.q).astype(f32).reshape(9), S.t.astype(f32), f32(S.s)


def scw_pose(est, pose2):
    """mg2oScw = gScm*gSmw (LoopClosing.cc:333-335), Converter::toCvMat, then the decomposition of ORBmatcher.cc:301-305 as
    pilotguru_amd.orb.sim3_pose states it: (Tcw [12] float, Ow [3] float)."""
    R2, t2, _ = pose_parts(pose2)
    cw = sim3_mul(est, Sim3(quat_from_matrix(R2.astype(f64)), t2.astype(f64), 1.0))
    sR, t = (cw.s * matrix_from_quat(cw.q)).astype(f32), cw.t.astype(f32)
    r0 = sR[0].astype(f64)
    with np.errstate(all="ignore"):
        scw = f32(np.sqrt((r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2]))
        a = f32(f64(1.0) / f64(scw))
        R, t = (sR * a).astype(f32), (t * a).astype(f32)
        Ow = [f32(f64(f32(f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1])) + f32(R[2, i] * t[2]))) * f64(-1.0)) for i in range(3)]
    return np.concatenate([R, t.reshape(3, 1)], 1).reshape(12), np.array(Ow, f32)


# ---------------------------------------------------------------- edges
class Edges:
    """Per correspondence: P1c, P2c [m][3], obs1, obs2 [m][2], w1, w2 [m] widened to double; i1, i2; the two cameras as doubles."""

    def __init__(self, P1, P2, obs1, obs2, w1, w2, i1, i2, cam1, cam2):
        d = lambda a, k: np.asarray(a, f32).astype(f64).reshape(-1, k)
        self.P1, self.P2, self.obs1, self.obs2 = d(P1, 3), d(P2, 3), d(obs1, 2), d(obs2, 2)
        self.w1, self.w2 = np.asarray(w1, f32).astype(f64), np.asarray(w2, f32).astype(f64)
        self.i1, self.i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
        self.cam1, self.cam2 = tuple(f64(f32(c)) for c in cam1), tuple(f64(f32(c)) for c in cam2)

    def __len__(self):
        return len(self.i1)


def edge_error(S, cam, X, obs):
    """obs - cam_map(project(S.map(X))) on arrays."""
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        rx, ry, rz = rotate(S.q, X[:, 0], X[:, 1], X[:, 2])
        x, y, z = S.s * rx + S.t[0], S.s * ry + S.t[1], S.s * rz + S.t[2]
        return obs[:, 0] - ((x / z) * fx + cx), obs[:, 1] - ((y / z) * fy + cy), (x, y, z)


def edge_chi2(e0, e1, w):
    with np.errstate(all="ignore"):
        return e0 * (w * e0) + e1 * (w * e1)


def huber(c2, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(c2)
        inl = c2 <= dsqr
        return np.where(inl, c2, 2.0 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def pair_errors(S, E, act=slice(None)):
    """computeError of both edges at S (the inverse recomputed): (e12_0, e12_1, e21_0, e21_1)."""
    a0, a1, _ = edge_error(S, E.cam1, E.P2[act], E.obs1[act])
    b0, b1, _ = edge_error(sim3_inverse(S), E.cam2, E.P1[act], E.obs2[act])
    return a0, a1, b0, b1


def numeric_jacobian(est, E, act, fix_scale, lm):
    """BaseBinaryEdge::linearizeOplus on the Sim3 vertex: (J12_0, J12_1, J21_0, J21_1), each [7][m]."""
    scalar = f64(1.0) / (2 * DELTA_NUM)
    J = [[], [], [], []]
    for d in range(7):
        add = np.zeros(7, f64)
        add[d] = DELTA_NUM
        p = pair_errors(oplus(est, add, fix_scale, lm), E, act)
        add[d] = -DELTA_NUM
        m = pair_errors(oplus(est, add, fix_scale, lm), E, act)
        for k in range(4):
            J[k].append(scalar * (p[k] - m[k]))
    return J


def analytic_jacobian(est, E, act, fix_scale):
    """The derivative of both errors by the left update at 0 (what the commented-out overrides would state)."""
    def proj_rows(pc, cam):
        x, y, z = pc
        zero = np.zeros_like(x)
        return (-cam[0] / z, zero, cam[0] * x / (z * z)), (zero, -cam[1] / z, cam[1] * y / (z * z))
    _, _, p = edge_error(est, E.cam1, E.P2[act], E.obs1[act])
    inv = sim3_inverse(est)
    _, _, q = edge_error(inv, E.cam2, E.P1[act], E.obs2[act])
    x, y, z = p
    zero, one = np.zeros_like(x), np.ones_like(x)
    # exp(u).map(p) = p + omega x p + upsilon + sigma p: dp/du = [-[p]x | I | p]
    dp = [(zero, -z, y), (z, zero, -x), (-y, x, zero), (one, zero, zero), (zero, one, zero), (zero, zero, one), (x, y, z)]
    X1 = E.P1[act]
    Rt = matrix_from_quat(est.q).T / est.s
    # (exp(u) S)^-1 = S^-1 exp(-u): dq/du = (1/s) R' [[X1]x | -I | -X1]
    cols1 = [(zero, X1[:, 2], -X1[:, 1]), (-X1[:, 2], zero, X1[:, 0]), (X1[:, 1], -X1[:, 0], zero), (-one, zero, zero), (zero, -one, zero),
             (zero, zero, -one), (-X1[:, 0], -X1[:, 1], -X1[:, 2])]
    dq = [tuple(Rt[r, 0] * c[0] + Rt[r, 1] * c[1] + Rt[r, 2] * c[2] for r in range(3)) for c in cols1]
    J = [[], [], [], []]
    for k, (rows, dv) in enumerate(((proj_rows(p, E.cam1), dp), (proj_rows(q, E.cam2), dq))):
        for d in range(7):
            for r in range(2):
                v = rows[r][0] * dv[d][0] + rows[r][1] * dv[d][1] + rows[r][2] * dv[d][2]
                J[2 * k + r].append(np.zeros_like(x) if fix_scale and d == 6 else v)
    return J


def _interleave(a, b, rules):
    if rules.edge_order == "blocked":
        return np.concatenate([a, b])
    out = np.empty((2 * a.shape[0],) + a.shape[1:], f64)
    out[0::2], out[1::2] = a, b
    return out


def active_chi2(S, E, act, delta, robust, order, rules):
    a0, a1, b0, b1 = pair_errors(S, E, act)
    c12, c21 = edge_chi2(a0, a1, E.w1[act]), edge_chi2(b0, b1, E.w2[act])
    if robust:
        c12, c21 = huber(c12, delta)[0], huber(c21, delta)[0]
    return esum(_interleave(c12, c21, rules), order)


def build_system(est, E, act, delta, robust, fix_scale, order, lm, rules):
    """computeActiveErrors, activeRobustChi2 and buildSystem: (H [7][7], b [7], chi2)."""
    a0, a1, b0, b1 = pair_errors(est, E, act)
    J = numeric_jacobian(est, E, act, fix_scale, lm) if rules.jacobian == "numeric" else analytic_jacobian(est, E, act, fix_scale)
    rows = []
    for e0, e1, w, J0, J1 in ((a0, a1, E.w1[act], J[0], J[1]), (b0, b1, E.w2[act], J[2], J[3])):
        c2 = edge_chi2(e0, e1, w)
        rho0, rho1 = huber(c2, delta) if robust else (c2, np.ones_like(c2))
        with np.errstate(all="ignore"):
            wr = rho1 * w
            r0, r1 = (-(w * e0)) * rho1, (-(w * e1)) * rho1
            cols = []
            for i in range(7):
                x0, x1 = J0[i] * wr, J1[i] * wr
                for j in range(i, 7):
                    cols.append(x0 * J0[j] + x1 * J1[j])
            for i in range(7):
                cols.append(J0[i] * r0 + J1[i] * r1)
            cols.append(rho0)
        rows.append(np.stack(cols, 1))
    with np.errstate(all="ignore"):
        s = esum(_interleave(rows[0], rows[1], rules), order)
    H = np.zeros((7, 7), f64)
    k = 0
    for i in range(7):
        for j in range(i, 7):
            H[i, j] = H[j, i] = s[k]
            k += 1
    return H, s[28:35].copy(), s[35]


def ldlt_solve(H, b):
    """LinearSolverDense: an LDLT in index order; (x, ok) with ok False when a factor is not positive."""
    n = len(b)
    L, d, ok = np.zeros((n, n), f64), np.zeros(n, f64), True
    with np.errstate(all="ignore"):
        for j in range(n):
            s = H[j, j]
            for k in range(j):
                s = s - (L[j, k] * L[j, k]) * d[k]
            d[j] = s
            ok = ok and bool(s > 0)
            for i in range(j + 1, n):
                t = H[j, i]
                for k in range(j):
                    t = t - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = t / s
        y = np.zeros(n, f64)
        for i in range(n):
            t = b[i]
            for k in range(i):
                t = t - L[i, k] * y[k]
            y[i] = t
        y = y / d
        x = np.zeros(n, f64)
        for i in range(n - 1, -1, -1):
            t = y[i]
            for k in range(i + 1, n):
                t = t - L[k, i] * x[k]
            x[i] = t
    return x, ok


class _LM:
    def __init__(self):
        self.lam, self.ni, self.nbad, self.started = 0.0, 2, 0, False


def optimize(est, E, act, iterations, delta, robust, fix_scale, order, lm, rules, hits, state, trace):
    """SparseOptimizer::optimize(iterations).  Returns (estimate, the estimate the active errors were last computed at, iterations
    run, trials), or None when the active chi2 is not finite.  trace receives one list of accept / reject flags per iteration."""
    err_est, its, trials = est, 0, 0
    if not act.any():
        return est, err_est, 0, 0
    accepted = True
    for it in range(iterations):
        H, b, current = build_system(est, E, act, delta, robust, fix_scale, order, lm, rules)
        ini = current
        if not np.isfinite(current):
            return None
        if it == 0 and (rules.lambda_reset or not state.started):
            state.lam, state.started = 1e-5 * max(0.0, max(abs(H[j, j]) for j in range(7))), True
        if it == 0:
            state.ni, state.nbad = 2, 0
        its += 1
        rho, qmax, row = 0.0, 0, []
        while True:
            Hl = H.copy()
            for j in range(7):
                Hl[j, j] = H[j, j] + state.lam
            x, ok = ldlt_solve(Hl, b)
            if not ok:
                x = np.zeros(7, f64)
            xs = x.copy()
            trial = oplus(est, x if rules.zero_x6 else xs, fix_scale, lm, hits)
            err_est = trial
            temp = active_chi2(trial, E, act, delta, robust, order, rules)
            if not ok:
                temp = DBL_MAX
            with np.errstate(all="ignore"):
                rho = current - temp
                scale = f64(0.0)
                for j in range(7):
                    scale = scale + x[j] * (state.lam * x[j] + b[j])
                scale = scale + 1e-3
                rho = rho / scale
            accepted = bool(rho > 0 and np.isfinite(temp))
            row.append(accepted)
            if accepted:
                t = 2.0 * rho - 1.0
                alpha = min(1.0 - (t * t) * t, 2.0 / 3.0)
                state.lam *= max(1.0 / 3.0, alpha)
                state.ni = 2
                current = temp
                est = trial
            else:
                hits["lm_rejected"] = hits.get("lm_rejected", 0) + 1
                state.lam *= float(state.ni)
                state.ni *= 2
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        trace.append(row)
        if qmax == 10 or rho == 0:
            hits["terminated"] = hits.get("terminated", 0) + 1
            break
        if (ini - current) * 1e3 < ini:
            state.nbad += 1
        else:
            state.nbad = 0
        if state.nbad >= 3:
            break
    if not accepted:
        hits["ended_on_rejected"] = hits.get("ended_on_rejected", 0) + 1
    return est, err_est, its, trials


def merged_matches(matches12, new_matches12, rules=REFERENCE):
    m = np.asarray(matches12, np.int32).copy()
    if new_matches12 is not None and rules.use_new_matches:
        nm = np.asarray(new_matches12, np.int32)
        m[nm >= 0] = nm[nm >= 0]
    return m


def gather(keys1, octaves1, pose1, kf_point1, keys2, octaves2, pose2, kf_point2, merged, points, bad, inv_sigma2):
    """The correspondences in i1 order (:1099-1178) as Edges."""
    keep = []
    for i1, i2 in enumerate(merged):
        if i2 < 0 or kf_point1[i1] < 0 or kf_point2[i2] < 0:
            continue
        if bad is not None and (bad[kf_point1[i1]] or bad[kf_point2[i2]]):
            continue
        keep.append((i1, int(i2)))
    i1 = np.array([a for a, _ in keep], np.int64)
    i2 = np.array([b for _, b in keep], np.int64)
    R1, t1, cam1 = pose_parts(pose1)
    R2, t2, cam2 = pose_parts(pose2)
    points = np.asarray(points, f32).reshape(-1, 3)
    P1 = gemm_rows(R1, t1, points[np.asarray(kf_point1)[i1]].reshape(-1, 3))
    P2 = gemm_rows(R2, t2, points[np.asarray(kf_point2)[i2]].reshape(-1, 3))
    k1, k2 = np.asarray(keys1, f32).reshape(-1, 2), np.asarray(keys2, f32).reshape(-1, 2)
    w = np.asarray(inv_sigma2, f32)
    return Edges(P1, P2, k1[i1], k2[i2], w[np.asarray(octaves1, np.int64)[i1]], w[np.asarray(octaves2, np.int64)[i2]], i1, i2, cam1, cam2)


def optimize_sim3(keys1, octaves1, pose1, kf_point1, keys2, octaves2, pose2, kf_point2, matches12, new_matches12, points, bad, estimate,
                  th2=10.0, fix_scale=False, inv_sigma2=None, form="edges", rules=REFERENCE, hits=None, trace=None):
    """estimate: (R [9], t [3], s) floats.  Returns a dict: ret (nIn), R [9], t [3], s (float), matches12_out [n1], chi2_12, chi2_21
    [n1] float, scw_Tcw [12], scw_Ow [3] (None with a status), status, ncorr, nbad, iterations [2], trials [2], more.  trace (a dict)
    receives lm = the accept / reject rows of both calls and cls = per classification (removed flags, chi2_12, chi2_21 in double)."""
    hits = {} if hits is None else hits
    trace = {} if trace is None else trace
    trace["lm"], trace["cls"] = [[], []], []
    order, lm = form_parts(form)
    inv_sigma2 = inv_level_sigma2() if inv_sigma2 is None else inv_sigma2
    merged = merged_matches(matches12, new_matches12, rules)
    n1 = len(merged)
    E = gather(keys1, octaves1, pose1, kf_point1, keys2, octaves2, pose2, kf_point2, merged, points, bad, inv_sigma2)
    m = len(E)
    th2f = f32(th2)
    th2d = f64(th2f)
    with np.errstate(all="ignore"):
        delta = f64(f32(np.sqrt(th2d)))                                 # const float deltaHuber = sqrt(th2)
    R_in, t_in, s_in = np.asarray(estimate[0], f32).reshape(9), np.asarray(estimate[1], f32).reshape(3), f32(estimate[2])
    out = dict(ret=0, R=R_in.copy(), t=t_in.copy(), s=s_in, matches12_out=merged.copy(), chi2_12=np.zeros(n1, f32), chi2_21=np.zeros(n1, f32),
               scw_Tcw=None, scw_Ow=None, status=0, ncorr=m, nbad=0, iterations=[0, 0], trials=[0, 0], more=0)
    est = from_estimate(R_in, t_in, s_in)
    act = np.ones(m, bool)
    state = _LM()
    c12f, c21f = np.zeros(m, f64), np.zeros(m, f64)

    def nonfinite():
        hits["nonfinite"] = hits.get("nonfinite", 0) + 1
        out.update(status=OS3_NONFINITE, matches12_out=merged.copy(), chi2_12=np.zeros(n1, f32), chi2_21=np.zeros(n1, f32))
        return out

    removed_any = np.zeros(m, bool)
    for call in range(2):
        iterations = 5 if call == 0 else out["more"]
        robust = True if call == 0 else rules.huber_second
        r = optimize(est, E, act, iterations, delta, robust, bool(fix_scale), order, lm, rules, hits, state, trace["lm"][call])
        if r is None:
            return nonfinite()
        est, err_est, out["iterations"][call], out["trials"][call] = r
        a0, a1, b0, b1 = pair_errors(err_est if rules.stale_read else est, E)
        c12, c21 = edge_chi2(a0, a1, E.w1), edge_chi2(b0, b1, E.w2)
        if not (np.isfinite(c12[act]).all() and np.isfinite(c21[act]).all()):
            return nonfinite()
        with np.errstate(all="ignore"):
            over = ((c12 >= th2d) | (c21 >= th2d)) if rules.remove_ge else ((c12 > th2d) | (c21 > th2d))
        over &= act
        trace["cls"].append((over.copy(), np.where(act, c12, 0.0), np.where(act, c21, 0.0), act.copy()))
        c12f, c21f = np.where(act, c12, c12f), np.where(act, c21, c21f)
        removed_any |= over
        if call == 0:
            out["nbad"] = int(over.sum())
            act = act & ~over
            out["more"] = rules.more_iterations[0] if out["nbad"] > 0 else rules.more_iterations[1]
            left = m - out["nbad"]
            if (left <= 10) if rules.few_le else (left < 10):
                hits["few"] = hits.get("few", 0) + 1
                out["status"] = OS3_FEW
                break
        else:
            out["ret"] = int((act & ~over).sum())
    out["matches12_out"][E.i1[removed_any]] = -1
    out["chi2_12"][E.i1] = c12f.astype(f32)
    out["chi2_21"][E.i1] = c21f.astype(f32)
    if out["status"] == 0 or rules.write_on_few:
        out["R"], out["t"], out["s"] = to_estimate(est)
    if out["status"] == 0:
        out["scw_Tcw"], out["scw_Ow"] = scw_pose(est, pose2)
    out["final"] = est
    return out
