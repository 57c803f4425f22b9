"""PnPsolver restated in plain Python: the definition that pilotguru_amd/csrc/pnp.hip follows operation by operation.

Restates thirdparty/orb-slam2/src/PnPsolver.cc:67-950 (the constructor, SetRansacParameters, iterate / find, Refine,
CheckInliers and the EPnP under compute_pose) under the readings of DESIGN.md section 4 (the PnPsolver rows):

  cvSVD / cvSolve(CV_SVD) / cvInvert(CV_SVD) on CV_64F are read as OpenCV 2.4's JacobiSVDImpl_<double>: one-sided Hestenes on the
  rows of A^T, cyclic (i, j) with i < j, skip when |p| <= 10*DBL_EPSILON*sqrt(a*b), the rotation from + - * / sqrt only
  (gamma = sqrt(p*p + beta*beta), no hypot), at most max(m, 30) sweeps, a selection sort to descending W with the rows
  following, each row then scaled by 1/W[i] when W[i] > DBL_MIN and left as it is otherwise.

A 4-point hypothesis depends on the null-space basis this routine happens to produce, so no tolerance compares one: every
double of the hypothesis stage (draw, compute_pose, CheckInliers count) is formed here in the order the device uses, and the
device is compared byte for byte.  `form` selects how Refine's long sums over the n correspondences are reduced ("seq": from 0
in order, the device's shape too; "pair": pairwise halves) and exists only to record a spread.

Every function takes `mut`, a set of names from MUTANTS: the rule changes the tests must be able to see.
"""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
NAN = float("nan")

FEW, FOUND, NO_MORE, REFINED = 1, 2, 4, 8

MUTANTS = (
    "loop_and",            # && for the || of iterate's loop condition
    "refine_ge",           # Refine returns true for refined >= min
    "refine_current",      # Refine runs on the current set, not the best
    "improve_ge",          # the best set is replaced for inl >= best
    "sign_mean_depth",     # solve_for_sign on the mean depth, not pcs[2] of the first correspondence
    "no_det_flip",         # estimate_R_and_t without the det < 0 row flip
    "epsilon_not_raised",  # epsilon stays as passed
    "min_rounded",         # int(N*eps) rounded, not truncated
    "check_double",        # CheckInliers all in double
)


def f32(x):
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def div(a, b):
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -math.inf if neg else math.inf
    return a / b


def sq(x):
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def lsum(terms, form="seq"):
    """a long sum: "seq" from 0.0 in order; "pair" pairwise halves"""
    if form == "seq":
        s = 0.0
        for t in terms:
            s += t
        return s
    n = len(terms)
    if n == 0:
        return 0.0
    if n == 1:
        return 0.0 + terms[0]
    h = n // 2
    return lsum(terms[:h], form) + lsum(terms[h:], form)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def dist2(a, b):
    return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])


# ---- JacobiSVDImpl_<double> -------------------------------------------------------------------------------------------------
def jacobi_svd(At, want_v):
    """At: n rows of length m (the rows of A^T).  Returns W[n] descending, the rows scaled to unit length (U^T), Vt or None."""
    n, m = len(At), len(At[0])
    At = [list(map(float, r)) for r in At]
    Vt = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)] if want_v else None
    eps = DBL_EPSILON * 10
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a = b = p = 0.0
                for k in range(m):
                    a += Ai[k] * Ai[k]
                    b += Aj[k] * Aj[k]
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * sq(a * b):
                    continue
                p *= 2.0
                beta = a - b
                gamma = sq(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = sq(div(delta, gamma))
                    c = div(p, (gamma * s) * 2.0)
                else:
                    c = sq(div(gamma + beta, gamma * 2.0))
                    s = div(p, (gamma * c) * 2.0)
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = (-s) * Ai[k] + c * Aj[k]
                    Ai[k] = t0
                    Aj[k] = t1
                if Vt is not None:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = (-s) * Vi[k] + c * Vj[k]
                        Vi[k] = t0
                        Vj[k] = t1
                changed = True
        if not changed:
            break
    W = []
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W.append(sq(sd))
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if Vt is not None:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    for i in range(n):
        if W[i] > DBL_MIN:
            s = div(1.0, W[i])
            At[i] = [x * s for x in At[i]]
    return W, At, Vt


def svd_solve(L, rho):
    """cvSolve(L, rho, x, CV_SVD) for a 6 x nc L: SVBkSb with threshold = DBL_EPSILON * sum(w)"""
    nr, nc = len(L), len(L[0])
    W, Ut, Vt = jacobi_svd([[L[r][c] for r in range(nr)] for c in range(nc)], True)
    thr = 0.0
    for i in range(nc):
        thr += W[i]
    thr *= DBL_EPSILON
    x = [0.0] * nc
    for i in range(nc):
        wi = W[i]
        if abs(wi) <= thr:
            continue
        wi = div(1.0, wi)
        s = 0.0
        for j in range(nr):
            s += Ut[i][j] * rho[j]
        s *= wi
        for j in range(nc):
            x[j] = x[j] + s * Vt[i][j]
    return x


def svd_invert3(CC):
    """cvInvert(CC, inv, CV_SVD): inv[r][c] = sum_i Vt[i][r] * (U[c][i] * (1/w_i)), i in order, the same threshold"""
    W, Ut, Vt = jacobi_svd([[CC[r][c] for r in range(3)] for c in range(3)], True)
    thr = ((0.0 + W[0]) + W[1]) + W[2]
    thr *= DBL_EPSILON
    inv = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        wi = W[i]
        if abs(wi) <= thr:
            continue
        wi = div(1.0, wi)
        buf = [Ut[i][c] * wi for c in range(3)]
        for r in range(3):
            for c in range(3):
                inv[r][c] = inv[r][c] + Vt[i][r] * buf[c]
    return inv


def qr_solve(A, b, X):
    """PnPsolver::qr_solve (:860-950) on an nr x nc A (rows), in place on A and b; False (X untouched) on eta == 0"""
    nr, nc = len(A), len(A[0])
    A1 = [0.0] * nc
    A2 = [0.0] * nc
    for k in range(nc):
        # the reference's scan reads before it steps: rows k .. nr-2
        eta = abs(A[k][k])
        for i in range(k, nr - 1):
            elt = abs(A[i][k])
            if eta < elt:
                eta = elt
        if eta == 0:
            return False
        inv_eta = div(1.0, eta)
        s = 0.0
        for i in range(k, nr):
            A[i][k] *= inv_eta
            s += A[i][k] * A[i][k]
        sigma = sq(s)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] += sigma
        A1[k] = sigma * A[k][k]
        A2[k] = (-eta) * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i][k] * A[i][j]
            tau = div(s, A1[k])
            for i in range(k, nr):
                A[i][j] -= tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i][j] * b[i]
        tau = div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i][j]
    X[nc - 1] = div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i][j] * X[j]
        X[i] = div(b[i] - s, A2[i])
    return True


def gauss_newton(L, rho, betas):
    x = [0.0] * 4              # READ: X starts as zeros (the reference leaves it uninitialised before the first solve)
    for _ in range(5):
        A = []
        b = []
        for i in range(6):
            r = L[i]
            A.append([
                (((2 * r[0]) * betas[0] + r[1] * betas[1]) + r[3] * betas[2]) + r[6] * betas[3],
                ((r[1] * betas[0] + (2 * r[2]) * betas[1]) + r[4] * betas[2]) + r[7] * betas[3],
                ((r[3] * betas[0] + r[4] * betas[1]) + (2 * r[5]) * betas[2]) + r[8] * betas[3],
                ((r[6] * betas[0] + r[7] * betas[1]) + r[8] * betas[2]) + (2 * r[9]) * betas[3]])
            q = (r[0] * betas[0]) * betas[0]
            q += (r[1] * betas[0]) * betas[1]
            q += (r[2] * betas[1]) * betas[1]
            q += (r[3] * betas[0]) * betas[2]
            q += (r[4] * betas[1]) * betas[2]
            q += (r[5] * betas[2]) * betas[2]
            q += (r[6] * betas[0]) * betas[3]
            q += (r[7] * betas[1]) * betas[3]
            q += (r[8] * betas[2]) * betas[3]
            q += (r[9] * betas[3]) * betas[3]
            b.append(rho[i] - q)
        qr_solve(A, b, x)
        for i in range(4):
            betas[i] += x[i]


def betas_approx(which, L, rho):
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}[which]
    b = svd_solve([[L[i][c] for c in cols] for i in range(6)], rho)
    be = [0.0] * 4
    if which == 1:
        if b[0] < 0:
            be[0] = sq(-b[0])
            be[1] = div(-b[1], be[0]); be[2] = div(-b[2], be[0]); be[3] = div(-b[3], be[0])
        else:
            be[0] = sq(b[0])
            be[1] = div(b[1], be[0]); be[2] = div(b[2], be[0]); be[3] = div(b[3], be[0])
        return be
    if b[0] < 0:
        be[0] = sq(-b[0])
        be[1] = sq(-b[2]) if b[2] < 0 else 0.0
    else:
        be[0] = sq(b[0])
        be[1] = sq(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        be[0] = -be[0]
    be[2] = div(b[3], be[0]) if which == 3 else 0.0
    return be


def compute_pose(pws, us, cam, mut=frozenset(), form="seq"):
    """PnPsolver::compute_pose (:477-525): pws [n][3], us [n][2] doubles, cam = (fu, fv, uc, vc).  Returns R (9), t (3), error."""
    fu, fv, uc, vc = (float(v) for v in cam)
    n = len(pws)
    nd = float(n)
    # choose_control_points
    cws = [[0.0] * 3 for _ in range(4)]
    for j in range(3):
        cws[0][j] = div(lsum([pws[i][j] for i in range(n)], form), nd)
    pw0tpw0 = [[lsum([(pws[i][r] - cws[0][r]) * (pws[i][c] - cws[0][c]) for i in range(n)], form) for c in range(3)] for r in range(3)]
    dc, uct, _ = jacobi_svd(pw0tpw0, False)          # symmetric: the rows of A^T are A's rows
    for i in range(1, 4):
        k = sq(div(dc[i - 1], nd))
        for j in range(3):
            cws[i][j] = cws[0][j] + k * uct[i - 1][j]
    # compute_barycentric_coordinates
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = svd_invert3(cc)
    alphas = []
    for i in range(n):
        p = pws[i]
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = (ci[j][0] * (p[0] - cws[0][0]) + ci[j][1] * (p[1] - cws[0][1])) + ci[j][2] * (p[2] - cws[0][2])
        a[0] = ((1.0 - a[1]) - a[2]) - a[3]
        alphas.append(a)
    # fill_M and cvMulTransposed(M, MtM, 1): sums over the rows in row order
    M = []
    for i in range(n):
        a = alphas[i]
        u, v = us[i]
        r1, r2 = [], []
        for k in range(4):
            r1 += [a[k] * fu, 0.0, a[k] * (uc - u)]
            r2 += [0.0, a[k] * fv, a[k] * (vc - v)]
        M.append(r1)
        M.append(r2)
    mtm = [[lsum([M[r][i] * M[r][j] for r in range(2 * n)], form) for j in range(12)] for i in range(12)]
    _, ut, _ = jacobi_svd(mtm, False)
    # compute_L_6x10, compute_rho
    v = [ut[11], ut[10], ut[9], ut[8]]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    dv = [[[v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)] for (a, b) in pairs] for i in range(4)]
    L = []
    for i in range(6):
        L.append([dot3(dv[0][i], dv[0][i]), 2.0 * dot3(dv[0][i], dv[1][i]), dot3(dv[1][i], dv[1][i]), 2.0 * dot3(dv[0][i], dv[2][i]),
                  2.0 * dot3(dv[1][i], dv[2][i]), dot3(dv[2][i], dv[2][i]), 2.0 * dot3(dv[0][i], dv[3][i]), 2.0 * dot3(dv[1][i], dv[3][i]),
                  2.0 * dot3(dv[2][i], dv[3][i]), dot3(dv[3][i], dv[3][i])])
    rho = [dist2(cws[a], cws[b]) for (a, b) in pairs]
    cand = []
    for which in (1, 2, 3):
        betas = betas_approx(which, L, rho)
        gauss_newton(L, rho, betas)
        cand.append(compute_R_and_t(v, betas, alphas, pws, us, (fu, fv, uc, vc), mut, form))
    N = 0
    if cand[1][2] < cand[0][2]:
        N = 1
    if cand[2][2] < cand[N][2]:
        N = 2
    return cand[N]


def compute_R_and_t(v, betas, alphas, pws, us, cam, mut, form):
    fu, fv, uc, vc = cam
    n = len(pws)
    nd = float(n)
    ccs = [[0.0] * 3 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            for k in range(3):
                ccs[j][k] += betas[i] * v[i][3 * j + k]
    pcs = []
    for i in range(n):
        a = alphas[i]
        pcs.append([((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j] for j in range(3)])
    # solve_for_sign: the depth of the FIRST correspondence only
    depth = pcs[0][2] if n else 0.0
    if "sign_mean_depth" in mut and n:
        depth = div(lsum([p[2] for p in pcs]), nd)
    if depth < 0.0:
        pcs = [[-p[0], -p[1], -p[2]] for p in pcs]
    # estimate_R_and_t
    pc0 = [div(lsum([pcs[i][j] for i in range(n)], form), nd) for j in range(3)]
    pw0 = [div(lsum([pws[i][j] for i in range(n)], form), nd) for j in range(3)]
    abt = [[lsum([(pcs[i][j] - pc0[j]) * (pws[i][c] - pw0[c]) for i in range(n)], form) for c in range(3)] for j in range(3)]
    _, Ut, Vt = jacobi_svd([[abt[r][c] for r in range(3)] for c in range(3)], True)
    U = [[Ut[k][i] for k in range(3)] for i in range(3)]          # abt_u's rows
    V = [[Vt[k][j] for k in range(3)] for j in range(3)]          # abt_v's rows
    R = [[dot3(U[i], V[j]) for j in range(3)] for i in range(3)]
    det = (R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]
    det = det + (R[0][2] * R[1][0]) * R[2][1]
    det = det - (R[0][2] * R[1][1]) * R[2][0]
    det = det - (R[0][1] * R[1][0]) * R[2][2]
    det = det - (R[0][0] * R[1][2]) * R[2][1]
    if det < 0 and "no_det_flip" not in mut:
        R[2] = [-R[2][0], -R[2][1], -R[2][2]]
    t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
    # reprojection_error
    terms = []
    for i in range(n):
        pw = pws[i]
        Xc = dot3(R[0], pw) + t[0]
        Yc = dot3(R[1], pw) + t[1]
        inv_Zc = div(1.0, dot3(R[2], pw) + t[2])
        ue = uc + (fu * Xc) * inv_Zc
        ve = vc + (fv * Yc) * inv_Zc
        u, w = us[i]
        terms.append(sq((u - ue) * (u - ue) + (w - ve) * (w - ve)))
    err = div(lsum(terms, form), nd)
    return [R[0][0], R[0][1], R[0][2], R[1][0], R[1][1], R[1][2], R[2][0], R[2][1], R[2][2]], t, err


# ---- the solver around it ----------------------------------------------------------------------------------------------------
def ransac(probability, min_inliers, max_iterations, min_set, epsilon, N, mut=frozenset()):
    """SetRansacParameters (:121-157): (adjusted mRansacMinInliers, mRansacMaxIts).  probability and epsilon are floats."""
    prob = float(np.float32(probability))
    eps = np.float32(epsilon)
    prod = np.float32(N) * eps
    n_min = int(round(float(prod))) if "min_rounded" in mut else int(float(prod))
    n_min = max(n_min, min_inliers)
    n_min = max(n_min, min_set)
    with np.errstate(all="ignore"):
        ratio = np.float32(n_min) / np.float32(N)
    if "epsilon_not_raised" not in mut and eps < ratio:
        eps = ratio
    if n_min == N:
        nit = 1
    else:
        e = float(eps)
        try:
            val = math.ceil(math.log(1 - prob) / math.log(1 - math.pow(e, 3)))
        except (ValueError, ZeroDivisionError, OverflowError):
            val = None
        nit = -2147483648 if val is None or not (-2147483648.0 <= val < 2147483648.0) else int(val)
    return n_min, max(1, min(nit, max_iterations))


def random_int(r, size):
    return int((r / 2147483648.0) * size)


def select_literal(draws, N):
    avail = list(range(N))
    out = []
    for r in draws:
        k = random_int(int(r), len(avail))
        out.append(avail[k])
        avail[k] = avail[-1]
        avail.pop()
    return out


def select_closed(draws, N):
    """the same without the list: the positions a swap has overwritten are kept, every other position holds its own index"""
    pos, val, out = [], [], []

    def content(q):
        for a in range(len(pos) - 1, -1, -1):
            if pos[a] == q:
                return val[a]
        return q
    size = N
    for r in draws:
        k = random_int(int(r), size)
        out.append(content(k))
        back = content(size - 1)
        pos.append(k)
        val.append(back)
        size -= 1
    return out


def correspondences(kps, kp_point, points, point_bad, sigma2, th2):
    """the constructor (:78-101): X (float), u, v (float), maxError = sigma2[octave]*th2 (float), the keypoint index"""
    rec = []
    npoints = len(points)
    for i in range(len(kp_point)):
        s = int(kp_point[i])
        if s < 0 or s >= npoints:
            continue
        if point_bad is not None and point_bad[s]:
            continue
        o = int(kps[i]["octave"])
        if o < 0 or o >= len(sigma2):
            continue
        me = np.float32(sigma2[o]) * np.float32(th2)
        rec.append((float(np.float32(points[s][0])), float(np.float32(points[s][1])), float(np.float32(points[s][2])),
                    float(np.float32(kps[i]["x"])), float(np.float32(kps[i]["y"])), float(me), i))
    return rec


def check_inliers(R, t, rec, cam, mut=frozenset(), want_error=False):
    """CheckInliers (:308-339) in its mixed types over all records at once (elementwise, so the order of records is immaterial)"""
    fu, fv, uc, vc = (float(v) for v in cam)
    if not rec:
        return np.zeros(0, bool)
    A = np.array([r[:6] for r in rec], np.float64)
    X, Y, Z, u, v, me = A.T
    f = (lambda a: a) if "check_double" in mut else (lambda a: a.astype(np.float32))
    d = lambda a: a.astype(np.float64)
    R = [np.float64(x) for x in R]
    t = [np.float64(x) for x in t]
    with np.errstate(all="ignore"):
        Xc = f(((R[0] * X + R[1] * Y) + R[2] * Z) + t[0])
        Yc = f(((R[3] * X + R[4] * Y) + R[5] * Z) + t[1])
        iz = f(1.0 / (((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]))
        ue = uc + (fu * d(Xc)) * d(iz)
        ve = vc + (fv * d(Yc)) * d(iz)
        dx = f(u - ue)
        dy = f(v - ve)
        e2 = dx * dx + dy * dy
        inl = e2 < f(me)
    if want_error:
        return inl, e2
    return inl


def hypothesis(rec, cam, draws4, mut=frozenset()):
    """one iteration of iterate's loop up to the count: R, t (doubles), count, mask"""
    idx = select_closed(draws4, len(rec))
    pws = [rec[i][0:3] for i in idx]
    us = [rec[i][3:5] for i in idx]
    R, t, _ = compute_pose(pws, us, cam, mut)
    inl = check_inliers(R, t, rec, cam, mut)
    return R, t, int(inl.sum()), inl


def refine(rec, cam, mask, mut=frozenset(), form="seq"):
    """Refine (:260-305) on the set `mask`: R, t, refined count, refined mask"""
    sel = [r for r, m in zip(rec, mask) if m]
    R, t, _ = compute_pose([r[0:3] for r in sel], [r[3:5] for r in sel], cam, mut, form)
    inl = check_inliers(R, t, rec, cam, mut)
    return R, t, int(inl.sum()), inl


def pose_f32(R, t):
    return [f32(x) for x in R], [f32(x) for x in t]


class State:
    """what a solver carries between calls"""
    def __init__(self, N):
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(N, bool)
        self.best_pose = None            # (R float, t float)

    def copy(self):
        s = State(len(self.best_mask))
        s.iterations, s.best_inliers, s.best_mask, s.best_pose = self.iterations, self.best_inliers, self.best_mask.copy(), self.best_pose
        return s


def window(cap, first, niterations):
    return max(cap - first, niterations)


def _result(rec, status, n_min, cap, st, pose, mask, returned, refined=None):
    return {"status": status, "N": len(rec), "min_inliers": n_min, "cap": cap, "iterations": st.iterations,
            "ninliers": int(mask.sum()) if pose is not None else 0, "best_inliers": st.best_inliers, "returned": returned,
            "pose": pose, "mask": mask if pose is not None else np.zeros(len(rec), bool), "state": st, "refined": refined}


def iterate_literal(rec, cam, params, draws, state, mut=frozenset(), form="seq", hyps=None):
    """iterate (:165-258) as written.  params = (probability, min_inliers, max_iterations, min_set, epsilon, niterations);
    draws [window][min_set]; hyps (optional) = precomputed hypothesis() results per iteration of the window."""
    prob, min_inl, max_its, min_set, eps, nit = params
    N = len(rec)
    n_min, cap = ransac(prob, min_inl, max_its, min_set, eps, N, mut)
    st = state.copy()
    if N < n_min:
        return _result(rec, FEW | NO_MORE, n_min, cap, st, None, None, -1)
    cur = 0
    seen = []                        # the hypotheses this call evaluated: (R, t, count)
    cond = (lambda: st.iterations < cap and cur < nit) if "loop_and" in mut else (lambda: st.iterations < cap or cur < nit)
    while cond():
        k = cur
        cur += 1
        st.iterations += 1
        R, t, cnt, inl = hyps[k] if hyps is not None else hypothesis(rec, cam, draws[k], mut)
        seen.append((R, t, cnt))
        if cnt >= n_min:
            if cnt >= st.best_inliers if "improve_ge" in mut else cnt > st.best_inliers:
                st.best_mask = inl.copy()
                st.best_inliers = cnt
                st.best_pose = pose_f32(R, t)
            Rr, tr, rc, rmask = refine(rec, cam, inl if "refine_current" in mut else st.best_mask, mut, form)
            if rc >= n_min if "refine_ge" in mut else rc > n_min:
                return dict(_result(rec, FOUND | REFINED, n_min, cap, st, pose_f32(Rr, tr), rmask, state.iterations + k, (Rr, tr)), seen=seen)
    if st.iterations >= cap:
        if st.best_inliers >= n_min and st.best_pose is not None:
            return dict(_result(rec, FOUND | NO_MORE, n_min, cap, st, st.best_pose, st.best_mask, -1), seen=seen)
        return dict(_result(rec, NO_MORE, n_min, cap, st, None, None, -1), seen=seen)
    return dict(_result(rec, 0, n_min, cap, st, None, None, -1), seen=seen)


def iterate_scan(rec, cam, params, draws, state, hyps=None):
    """the device's form: every hypothesis of the window first, then Refine only where the best set changes (once for a carried
    set when a qualifying iteration comes before the first improvement)"""
    prob, min_inl, max_its, min_set, eps, nit = params
    N = len(rec)
    n_min, cap = ransac(prob, min_inl, max_its, min_set, eps, N)
    st = state.copy()
    if N < n_min:
        return _result(rec, FEW | NO_MORE, n_min, cap, st, None, None, -1)
    W = window(cap, st.iterations, nit)
    if hyps is None:
        hyps = [hypothesis(rec, cam, draws[k]) for k in range(W)]
    first = st.iterations
    known = None                     # Refine's result on the current best set
    for k in range(W):
        st.iterations = first + k + 1
        R, t, cnt, inl = hyps[k]
        if cnt < n_min:
            continue
        if cnt > st.best_inliers:
            st.best_mask, st.best_inliers, st.best_pose = inl.copy(), cnt, pose_f32(R, t)
            known = None
        if known is None:
            known = refine(rec, cam, st.best_mask)
        if known[2] > n_min:
            return _result(rec, FOUND | REFINED, n_min, cap, st, pose_f32(known[0], known[1]), known[3], first + k, (known[0], known[1]))
    if st.iterations >= cap:
        if st.best_inliers >= n_min and st.best_pose is not None:
            return _result(rec, FOUND | NO_MORE, n_min, cap, st, st.best_pose, st.best_mask, -1)
        return _result(rec, NO_MORE, n_min, cap, st, None, None, -1)
    return _result(rec, 0, n_min, cap, st, None, None, -1)


def camera_centre(Rf, tf):
    """Frame::SetPose's mOw = -Rcw.t()*tcw: the float dot on gemm's small-matrix path, times alpha = -1 in double, to float"""
    ow = []
    for i in range(3):
        a = np.float32(Rf[i]) * np.float32(tf[0])
        a = a + np.float32(Rf[3 + i]) * np.float32(tf[1])
        a = a + np.float32(Rf[6 + i]) * np.float32(tf[2])
        ow.append(f32(float(a) * -1.0))
    return ow
