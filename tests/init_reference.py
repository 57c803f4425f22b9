"""Initializer restated with numpy scalars: the definition that pilotguru_amd/csrc/initializer.hip follows operation by operation.

Restates thirdparty/orb-slam2/src/Initializer.cc:33-929 (Initialize, FindHomography, FindFundamental, ComputeH21, ComputeF21,
CheckHomography, CheckFundamental, ReconstructF, ReconstructH, Triangulate, Normalize, CheckRT, DecomposeE), the constructive part
of Tracking::CreateInitialMapMonocular (src/Tracking.cc:633-680) and DUtils::Random::RandomInt, under the readings of DESIGN.md
section 4 (the Initializer rows).  Every float operation is one np.float32 operation, every double operation one np.float64
operation; nothing is left to numpy's promotion rules.

  cv::SVDecomp / cv::SVD::compute on CV_32F are read as OpenCV 2.4.9's JacobiSVDImpl_<float> (one-sided Hestenes on the rows of
  `At`, W and the inner products in double, the rotation's c and s narrowed to float, at most max(m, 30) sweeps, a selection
  sort to descending W that swaps the rows) followed by its completion loop: every row i < n1 is scaled by (float)(1/W[i]), and a
  row whose W is <= FLT_MIN -- or that does not exist because n1 > n -- is generated from cv::RNG(0x12345678) and two rounds of
  Gram-Schmidt.  Which matrix plays `At` depends on the shape (m >= n: the transpose; m < n: the matrix itself), which is why
  ComputeF21's vt.row(8) is the completion vector and not a Jacobi output.  The generation loop is bounded at COMPLETION_TRIES
  rounds (the reference's is a `while`); no case comes near the bound.

An 8-point hypothesis depends on these details to the last bit, so no tolerance compares one: the device is compared byte for byte.
The one exception is the parallax (acos), see `parallax_forms`.

`window` is the window-at-once form: every hypothesis of the call evaluated first and the sequential best-update applied
afterwards, as the device does; `initialize(..., form="loop")` is the literal loop.

Every function that has a rule the tests must be able to see takes `mut`, a set of names from MUTANTS.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
FLT_EPSILON2 = f32(2.384185791015625e-07)          # FLT_EPSILON*2
FLT_MIN = f64(1.1754943508222875e-38)
CV_PI = f64(3.1415926535897932384626433832795)
COMPLETION_TRIES = 4
MAX_ITERATIONS = 1024
INFO, FINFO = 17, 11

FEW, NO_MODEL, MODEL_H, MODEL_F, OK, DEGENERATE_H, AMBIGUOUS, FEW_GOOD, LOW_PARALLAX = 1, 2, 4, 8, 16, 32, 64, 128, 256
# info: status, N, best iteration H, inliers H, best iteration F, inliers F, chosen motion hypothesis, nGood[8], the chosen model's inliers,
# the return value
I_STATUS, I_N, I_BEST_H, I_INL_H, I_BEST_F, I_INL_F, I_CHOSEN, I_NGOOD, I_MODEL_INL, I_RET = 0, 1, 2, 3, 4, 5, 6, 7, 15, 16
# finfo: SH, SF, RH, parallax[8]
F_SH, F_SF, F_RH, F_PARALLAX = 0, 1, 2, 3

MUTANTS = (
    "normalize_matched",   # Normalize over the matched keypoints only
    "score_pairs",         # the score summed as (term 1 + term 2) per match
    "best_ge",             # >= for > at the best-hypothesis update
    "f_th_5991",           # CheckFundamental's inlier threshold at 5.991
    "f_row8_jacobi",       # ComputeF21's vt.row(8) taken from the Jacobi's Vt of A^T
    "idx50_no_min",        # vCosParallax[50] without the min (the last element when there are fewer)
    "best_good_ge",        # bestGood >= minTriangulated
    "similar_08",          # 0.8 for 0.7 in ReconstructF
    "second_09",           # 0.9 for 0.75 in ReconstructH
    "t_not_normalised",    # t without the division by its norm
)

Z, ONE = f32(0), f32(1)


def d(x):
    return f64(x)


# ---- the cv::Mat steps ----
def dot3f(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def small(t, alpha=None, c=None):
    """gemm's small-matrix epilogue: (float)(t*alpha + c*beta) in double (no C: + 0.0, so a -0 sum becomes +0)"""
    v = d(t) if alpha is None else d(t) * d(alpha)
    return f32(v + (d(0) if c is None else d(c)))


def mul33(A, B, alpha=None):
    """3 x 3 times 3 x 3, flags 0: the small path"""
    return [small(dot3f(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]), alpha) for i in range(3) for j in range(3)]


def mul33_bt(A, B):
    """A*B.t(): GEMMSingleMul<float, double>, sums in double from 0, rounded once"""
    out = []
    for i in range(3):
        for j in range(3):
            s = d(0)
            for k in range(3):
                s = s + d(A[3 * i + k]) * d(B[3 * j + k])
            out.append(f32(s))
    return out


def mul33_at(A, B):
    """A.t()*B: the same path"""
    out = []
    for i in range(3):
        for j in range(3):
            s = d(0)
            for k in range(3):
                s = s + d(A[3 * k + i]) * d(B[3 * k + j])
            out.append(f32(s))
    return out


def mul31(A, v, c=None):
    """3 x 3 times 3 x 1 (the small path; `c` folded in as gemm's C)"""
    return [small(dot3f(A[3 * i], A[3 * i + 1], A[3 * i + 2], v[0], v[1], v[2]), None, None if c is None else c[i]) for i in range(3)]


def inv33(M):
    """cv::invert's 3 x 3 closed form: the determinant and the cofactors in double; det == 0 gives the zero matrix"""
    m = [d(x) for x in M]

    def C(a, b, c, e):
        return m[a] * m[b] - m[c] * m[e]
    det = m[0] * C(4, 8, 5, 7)
    det = det - m[1] * (m[3] * m[8] - m[5] * m[6])
    det = det + m[2] * (m[3] * m[7] - m[4] * m[6])
    if not det != d(0):
        return [Z] * 9
    i = d(1) / det
    return [f32(C(4, 8, 5, 7) * i), f32(C(2, 7, 1, 8) * i), f32(C(1, 5, 2, 4) * i),
            f32(C(5, 6, 3, 8) * i), f32(C(0, 8, 2, 6) * i), f32(C(2, 3, 0, 5) * i),
            f32(C(3, 7, 4, 6) * i), f32(C(1, 6, 0, 7) * i), f32(C(0, 4, 1, 3) * i)]


def det33(m):
    """cv::determinant of a 3 x 3 CV_32F: det3 in float, widened"""
    return d(m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]))


def normd(v):
    s = d(0)
    for x in v:
        s = s + d(x) * d(x)
    return np.sqrt(s)


def dotd(a, b):
    s = d(0)
    for x, y in zip(a, b):
        s = s + d(x) * d(y)
    return s


def scale_by(v, s):
    """Mat / double and Mat *= double: convertTo with the float scale, x*(float)s + 0"""
    s = f32(s)
    return [x * s + Z for x in v]


def hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(d(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(d(1) + a * a)
    return d(0)


class RNG:
    """cv::RNG: the multiply-with-carry generator"""

    def __init__(self, state=0x12345678):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF


def jacobi(At, Vt=None):
    """JacobiSVDImpl_<float> up to and including the sort.  At: n rows of m float32 (modified); Vt: None or n rows of n, set to the
    identity here.  Returns W (double, descending)."""
    n, m = len(At), len(At[0])
    W = []
    for i in range(n):
        sd = d(0)
        for k in range(m):
            t = d(At[i][k])
            sd = sd + t * t
        W.append(sd)
        if Vt is not None:
            for k in range(n):
                Vt[i][k] = ONE if i == k else Z
    eps = d(FLT_EPSILON2)
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b, p = W[i], W[j], d(0)
                for k in range(m):
                    p = p + d(Ai[k]) * d(Aj[k])
                if abs(p) <= eps * np.sqrt(a * b):
                    continue
                p = p * d(2)
                beta = a - b
                gamma = hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * d(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * d(s) * d(2)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * d(2))))
                    s = f32(p / (gamma * d(c) * d(2)))
                a, b = d(0), d(0)
                ms = -s
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = ms * Ai[k] + c * Aj[k]
                    Ai[k], Aj[k] = t0, t1
                    a = a + d(t0) * d(t0)
                    b = b + d(t1) * d(t1)
                W[i], W[j] = a, b
                changed = True
                if Vt is not None:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = ms * Vi[k] + c * Vj[k]
                        Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = d(0)
        for k in range(m):
            t = d(At[i][k])
            sd = sd + t * t
        W[i] = np.sqrt(sd)
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
    return W


def complete(At, W, n1):
    """the completion loop: rows 0 .. n1-1 of `At` (rows from len(W) on are appended) normalised; generated where W <= FLT_MIN"""
    n, m = len(W), len(At[0])
    rng = RNG()
    while len(At) < n1:
        At.append([Z] * m)
    for i in range(n1):
        sd = W[i] if i < n else d(0)
        tries = 0
        while sd <= FLT_MIN and tries < COMPLETION_TRIES:
            tries += 1
            val0 = f32(d(1) / d(m))
            row = [val0 if (rng.next() & 256) != 0 else -val0 for _ in range(m)]
            for _ in range(2):
                for j in range(i):
                    Aj = At[j]
                    sd = d(0)
                    for k in range(m):
                        sd = sd + d(row[k] * Aj[k])
                    asum = Z
                    for k in range(m):
                        t = f32(d(row[k]) - sd * d(Aj[k]))
                        row[k] = t
                        asum = asum + abs(t)
                    asum = ONE / asum if asum != 0 else Z
                    for k in range(m):
                        row[k] = row[k] * asum
            At[i] = row
            sd = d(0)
            for k in range(m):
                t = d(row[k])
                sd = sd + t * t
            sd = np.sqrt(sd)
        s = f32(d(1) / sd)
        At[i] = [x * s for x in At[i]]
    return tries


def svd33(M):
    """cv::SVD::compute of a 3 x 3 (m = n: the Jacobi on the rows of M^T).  Returns (w [3] float, U [9], Vt [9])."""
    At = [[M[3 * k + i] for k in range(3)] for i in range(3)]
    Vt = [[Z] * 3 for _ in range(3)]
    W = jacobi(At, Vt)
    complete(At, W, 3)
    U = [At[c][r] for r in range(3) for c in range(3)]
    return [f32(x) for x in W], U, [x for row in Vt for x in row]


# ---- Initializer ----
def random_int(r, size):
    """DUtils::Random::RandomInt(0, size - 1) of a raw rand() value"""
    return int((d(int(r)) / d(2147483648.0)) * d(size))


def select_list(draws8, N):
    """the literal list (:84-96)"""
    avail = list(range(N))
    out = []
    for j in range(8):
        r = random_int(draws8[j], len(avail))
        r = min(max(r, 0), len(avail) - 1)             # (a draw >= 2^31: only the unchecked batched form can carry one)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def select_closed(draws8, N):
    """the same indices without the list: only the positions a swap has overwritten are kept"""
    pos, val, out = [], [], []
    size = N
    for j in range(8):
        r = random_int(draws8[j], size)
        r = min(max(r, 0), size - 1)
        pick, back = r, size - 1
        for a in range(j):
            if pos[a] == r:
                pick = val[a]
            if pos[a] == size - 1:
                back = val[a]
        out.append(pick)
        pos.append(r)
        val.append(back)
        size -= 1
    return out


def normalize(xy):
    """Normalize (:749-795) over ALL the keypoints given.  Returns (points [n][2], T [9])."""
    n = len(xy)
    mx, my = Z, Z
    for i in range(n):
        mx = mx + xy[i][0]
        my = my + xy[i][1]
    nf = f32(n)
    mx, my = mx / nf, my / nf
    dx, dy = Z, Z
    pts = []
    for i in range(n):
        x, y = xy[i][0] - mx, xy[i][1] - my
        pts.append((x, y))
        dx = dx + abs(x)
        dy = dy + abs(y)
    dx, dy = dx / nf, dy / nf
    sX, sY = f32(d(1) / d(dx)), f32(d(1) / d(dy))
    pts = [(x * sX, y * sY) for x, y in pts]
    return pts, [sX, Z, (-mx) * sX, Z, sY, (-my) * sY, Z, Z, ONE]


def compute_h21(p1, p2):
    At = [[Z] * 16 for _ in range(9)]
    for i in range(8):
        u1, v1 = p1[i]
        u2, v2 = p2[i]
        r0 = [Z, Z, Z, -u1, -v1, -ONE, v2 * u1, v2 * v1, v2]
        r1 = [u1, v1, ONE, Z, Z, Z, (-u2) * u1, (-u2) * v1, -u2]
        for c in range(9):
            At[c][2 * i] = r0[c]
            At[c][2 * i + 1] = r1[c]
    Vt = [[Z] * 9 for _ in range(9)]
    jacobi(At, Vt)
    return list(Vt[8])


def compute_f21(p1, p2, mut=()):
    rows = []
    for i in range(8):
        u1, v1 = p1[i]
        u2, v2 = p2[i]
        rows.append([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, ONE])
    if "f_row8_jacobi" in mut:
        At = [[rows[r][c] for r in range(8)] for c in range(9)]
        Vt = [[Z] * 9 for _ in range(9)]
        jacobi(At, Vt)
        pre = list(Vt[8])
    else:
        W = jacobi(rows)
        complete(rows, W, 9)
        pre = list(rows[8])
    w, U, Vt = svd33(pre)
    w[2] = Z
    D = [w[0], Z, Z, Z, w[1], Z, Z, Z, w[2]]
    return mul33(mul33(U, D), Vt)


TH = f32(5.991)
TH_F = f32(3.841)


def check_homography(H21, H12, m1, m2, sigma, mut=()):
    """CheckHomography (:305-388) over the matched coordinates m1[i], m2[i].  Returns (score, inlier flags)."""
    h, g = H21, H12
    inv_s2 = f32(d(1) / d(sigma * sigma))
    score = Z
    inl = []
    for i in range(len(m1)):
        u1, v1 = m1[i]
        u2, v2 = m2[i]
        ok = True
        w = f32(d(1) / d(g[6] * u2 + g[7] * v2 + g[8]))
        a = (g[0] * u2 + g[1] * v2 + g[2]) * w
        b = (g[3] * u2 + g[4] * v2 + g[5]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w = f32(d(1) / d(h[6] * u1 + h[7] * v1 + h[8]))
        a = (h[0] * u1 + h[1] * v1 + h[2]) * w
        b = (h[3] * u1 + h[4] * v1 + h[5]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        t1 = t2 = None
        if chi1 > TH:
            ok = False
        else:
            t1 = TH - chi1
        if chi2 > TH:
            ok = False
        else:
            t2 = TH - chi2
        score = _fold(score, t1, t2, mut)
        inl.append(ok)
    return score, inl


def _fold(score, t1, t2, mut):
    if "score_pairs" in mut:
        return score + ((Z if t1 is None else t1) + (Z if t2 is None else t2))
    if t1 is not None:
        score = score + t1
    if t2 is not None:
        score = score + t2
    return score


def check_fundamental(F, m1, m2, sigma, mut=()):
    """CheckFundamental (:390-468)"""
    f = F
    th = TH if "f_th_5991" in mut else TH_F
    inv_s2 = f32(d(1) / d(sigma * sigma))
    score = Z
    inl = []
    for i in range(len(m1)):
        u1, v1 = m1[i]
        u2, v2 = m2[i]
        ok = True
        a2 = f[0] * u1 + f[1] * v1 + f[2]
        b2 = f[3] * u1 + f[4] * v1 + f[5]
        c2 = f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = f[0] * u2 + f[3] * v2 + f[6]
        b1 = f[1] * u2 + f[4] * v2 + f[7]
        c1 = f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        t1 = t2 = None
        if chi1 > th:
            ok = False
        else:
            t1 = TH - chi1
        if chi2 > th:
            ok = False
        else:
            t2 = TH - chi2
        score = _fold(score, t1, t2, mut)
        inl.append(ok)
    return score, inl


def hypothesis(prep, sel, sigma, mut=()):
    """both models of one iteration on the set `sel`: a dict with H21, F21, scoreH, scoreF, inlH, inlF (flag lists)"""
    p1 = [prep["pn1"][prep["i1"][k]] for k in sel]
    p2 = [prep["pn2"][prep["i2"][k]] for k in sel]
    Hn = compute_h21(p1, p2)
    H21 = mul33(mul33(prep["T2inv"], Hn), prep["T1"])
    H12 = inv33(H21)
    sH, iH = check_homography(H21, H12, prep["m1"], prep["m2"], sigma, mut)
    Fn = compute_f21(p1, p2, mut)
    F21 = mul33(mul33(prep["T2t"], Fn), prep["T1"])
    sF, iF = check_fundamental(F21, prep["m1"], prep["m2"], sigma, mut)
    return dict(H21=H21, F21=F21, scoreH=sH, scoreF=sF, inlH=iH, inlF=iF, set=list(sel))


def prepare(k1, k2, matches12, mut=()):
    i1 = [i for i in range(len(matches12)) if matches12[i] >= 0]
    i2 = [int(matches12[i]) for i in i1]
    k1 = [(f32(x), f32(y)) for x, y in k1]
    k2 = [(f32(x), f32(y)) for x, y in k2]
    m1, m2 = [k1[i] for i in i1], [k2[i] for i in i2]
    if "normalize_matched" in mut:
        a, T1 = normalize(m1)
        b, T2 = normalize(m2)
        pn1, pn2 = {i: a[k] for k, i in enumerate(i1)}, {i: b[k] for k, i in enumerate(i2)}
    else:
        pn1, T1 = normalize(k1)
        pn2, T2 = normalize(k2)
    T2t = [T2[3 * c + r] for r in range(3) for c in range(3)]
    return dict(i1=i1, i2=i2, m1=m1, m2=m2, pn1=pn1, pn2=pn2, T1=T1, T2=T2, T2inv=inv33(T2), T2t=T2t, k1=k1, k2=k2)


def triangulate(x1, x2, P1, P2):
    """Triangulate (:734-747): the rows of A by addWeighted in double, the 4 x 4 SVD's vt.row(3), x/w by the float scale"""
    At = [[Z] * 4 for _ in range(4)]
    for c in range(4):
        At[c][0] = f32((d(P1[8 + c]) * d(x1[0]) + -d(P1[c])) + d(0))
        At[c][1] = f32((d(P1[8 + c]) * d(x1[1]) + -d(P1[4 + c])) + d(0))
        At[c][2] = f32((d(P2[8 + c]) * d(x2[0]) + -d(P2[c])) + d(0))
        At[c][3] = f32((d(P2[8 + c]) * d(x2[1]) + -d(P2[4 + c])) + d(0))
    Vt = [[Z] * 4 for _ in range(4)]
    jacobi(At, Vt)
    v = Vt[3]
    return scale_by(v[:3], d(1) / d(v[3]))


def parallax_forms(c):
    """acos(c)*180/CV_PI three ways: the reference's definition (the double acos of the float), float32 arccos, and atan2 of the
    sine and cosine in double.  The first is the definition; the spread among them bounds what a device's acos may differ by."""
    c = f32(c)
    a = f32(np.arccos(d(c)) * d(180) / CV_PI)
    b = f32(np.arccos(c) * f32(180) / f32(CV_PI))
    s = np.sqrt(max(d(0), d(1) - d(c) * d(c)))
    e = f32(np.arctan2(s, d(c)) * d(180) / CV_PI)
    return a, b, e


def check_rt(R, t, prep, inl, cam, th2, n1, mut=()):
    """CheckRT (:798-907).  Returns (nGood, parallax, P3D {i1: xyz}, good {i1: flag}, the sorted cosines)."""
    fx, fy, cx, cy = cam
    K = [fx, Z, cx, Z, fy, cy, Z, Z, ONE]
    P1 = [fx, Z, cx, Z, Z, fy, cy, Z, Z, Z, ONE, Z]
    RT = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    P2 = [small(dot3f(K[3 * i], K[3 * i + 1], K[3 * i + 2], RT[j], RT[4 + j], RT[8 + j])) for i in range(3) for j in range(4)]
    O2 = [f32(d(dot3f(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2])) * d(-1)) for i in range(3)]
    cosines, P3D, good = [], {}, {}
    nGood = 0
    lim = d(0.99998)
    for k in range(len(inl)):
        if not inl[k]:
            continue
        a, b = prep["m1"][k], prep["m2"][k]
        i1 = prep["i1"][k]
        X = triangulate(a, b, P1, P2)
        if not (np.isfinite(X[0]) and np.isfinite(X[1]) and np.isfinite(X[2])):
            good[i1] = False
            continue
        n1v = [X[0] - Z, X[1] - Z, X[2] - Z]
        dist1 = f32(normd(n1v))
        n2v = [X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]]
        dist2 = f32(normd(n2v))
        cosp = f32(dotd(n1v, n2v) / d(dist1 * dist2))
        if X[2] <= 0 and d(cosp) < lim:
            continue
        X2 = mul31(R, X, t)
        if X2[2] <= 0 and d(cosp) < lim:
            continue
        iz = f32(d(1) / d(X[2]))
        ex, ey = (fx * X[0] * iz + cx) - a[0], (fy * X[1] * iz + cy) - a[1]
        if ex * ex + ey * ey > th2:
            continue
        iz = f32(d(1) / d(X2[2]))
        ex, ey = (fx * X2[0] * iz + cx) - b[0], (fy * X2[1] * iz + cy) - b[1]
        if ex * ex + ey * ey > th2:
            continue
        cosines.append(cosp)
        P3D[i1] = X
        nGood += 1
        if d(cosp) < lim:
            good[i1] = True
    par = Z
    cosines.sort()
    if nGood > 0:
        idx = min(50, len(cosines) - 1)
        if "idx50_no_min" in mut:
            idx = 50 if len(cosines) > 50 else 0
        par = parallax_forms(cosines[idx])[0]
    return nGood, par, P3D, good, cosines


def decompose_e(E, mut=()):
    w, U, Vt = svd33(E)
    t = [U[2], U[5], U[8]]
    if "t_not_normalised" not in mut:
        t = scale_by(t, d(1) / normd(t))
    Wm = [Z, -ONE, Z, ONE, Z, Z, Z, Z, ONE]
    R1 = mul33(mul33(U, Wm), Vt)
    if det33(R1) < 0:
        R1 = [-x for x in R1]
    R2 = mul33(mul33_bt(U, Wm), Vt)
    if det33(R2) < 0:
        R2 = [-x for x in R2]
    return R1, R2, t


def reconstruct_f(F21, inl, prep, cam, sigma, min_parallax, min_tri, n1, mut=()):
    fx, fy, cx, cy = cam
    K = [fx, Z, cx, Z, fy, cy, Z, Z, ONE]
    N = sum(1 for x in inl if x)
    E = mul33(mul33_at(K, F21), K)
    R1, R2, t = decompose_e(E, mut)
    t2 = [-x for x in t]
    th2 = f32(d(4.0) * d(sigma * sigma))
    hyps = [(R1, t), (R2, t), (R1, t2), (R2, t2)]
    res = [check_rt(R, tt, prep, inl, cam, th2, n1, mut) for R, tt in hyps]
    ng = [r[0] for r in res]
    maxGood = max(ng)
    nMinGood = max(int(d(0.9) * d(N)), min_tri)
    lim = d(0.8 if "similar_08" in mut else 0.7) * d(maxGood)
    nsimilar = sum(1 for g in ng if d(g) > lim)
    status = 0
    if maxGood < nMinGood:
        status |= FEW_GOOD
    if nsimilar > 1:
        status |= AMBIGUOUS
    chosen = ng.index(maxGood)
    if not status:
        if res[chosen][1] > min_parallax:
            status |= OK
        else:
            status |= LOW_PARALLAX
    return status, chosen, hyps, res, N


def reconstruct_h(H21, inl, prep, cam, sigma, min_parallax, min_tri, n1, mut=()):
    fx, fy, cx, cy = cam
    K = [fx, Z, cx, Z, fy, cy, Z, Z, ONE]
    N = sum(1 for x in inl if x)
    A = mul33(mul33(inv33(K), H21), K)
    w, U, Vt = svd33(A)
    s = f32(det33(U) * det33(Vt))
    d1, d2, d3 = w
    if d(d1 / d2) < d(1.00001) or d(d2 / d3) < d(1.00001):
        return DEGENERATE_H, -1, [], [], N
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [aux_st, -aux_st, -aux_st, aux_st]
    aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
    hyps = []
    for i in range(8):
        q = i & 3
        if i < 4:
            Rp = [ct, Z, -st[q], Z, ONE, Z, st[q], Z, ct]
            tp = scale_by([x1[q], Z, -x3[q]], d(d1 - d3))
        else:
            Rp = [cp, Z, sp[q], Z, -ONE, Z, sp[q], Z, -cp]
            tp = scale_by([x1[q], Z, x3[q]], d(d1 + d3))
        R = mul33(mul33(U, Rp, alpha=s), Vt)
        t = mul31(U, tp)
        if "t_not_normalised" not in mut:
            t = scale_by(t, d(1) / normd(t))
        hyps.append((R, t))
    th2 = f32(d(4.0) * d(sigma * sigma))
    res = [check_rt(R, t, prep, inl, cam, th2, n1, mut) for R, t in hyps]
    best, second, idx, bestPar = 0, 0, -1, f32(-1)
    for i in range(8):
        g = res[i][0]
        if g > best:
            second, best, idx, bestPar = best, g, i, res[i][1]
        elif g > second:
            second = g
    status = 0
    if not d(second) < d(0.9 if "second_09" in mut else 0.75) * d(best):
        status |= AMBIGUOUS
    if not bestPar >= min_parallax:
        status |= LOW_PARALLAX
    if not (best >= min_tri if "best_good_ge" in mut else best > min_tri) or not d(best) > d(0.9) * d(N):
        status |= FEW_GOOD
    if not status:
        status = OK
    return status, idx, hyps, res, N


def put_pose(cam, R, t):
    """a pgorb_kf_pose as 21 floats: [R | t], Ow = -R.t()*t on gemm's small path with alpha -1, the camera copied, 1/fx, 1/fy"""
    T = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    Ow = [f32(d(dot3f(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2])) * d(-1)) for i in range(3)]
    return np.array(T + Ow + list(cam), f32)


def window(prep, draws, iters, sigma, mut=()):
    """every hypothesis of the call (the device's second launch)"""
    N = len(prep["i1"])
    return [hypothesis(prep, select_closed(draws[it], N), sigma, mut) for it in range(iters)]


def first_strict_maximum(scores, mut=()):
    """the sequential update (:165, :216) over the window's scores: (best iteration or -1, score)"""
    best, score = -1, Z
    for it, s in enumerate(scores):
        if (s >= score and s > 0) if "best_ge" in mut else s > score:
            best, score = it, s
    return best, score


def initialize(k1, k2, camera, matches12, sigma, iters, min_parallax, min_tri, draws, f1=0, f2=1, mut=(), form="window"):
    """Initializer::Initialize with Tracking.cc:612-626 and the constructive part of CreateInitialMapMonocular.

    k1 [n1][2], k2 [n2][2]: the undistorted keypoints; camera: 6 floats (fx, fy, cx, cy, invfx, invfy), copied into the poses;
    draws [iters][8] raw rand() values.  Returns a dict: ret, trace (a list of hypothesis dicts), pose (2 x 21 float32), P3D [n1][3],
    triangulated [n1], matches12_out [n1], points [np][3], kf_point1, kf_point2, obs_start, obs_frame, obs_idx, info, finfo."""
    with np.errstate(all="ignore"):
        return _initialize(k1, k2, camera, matches12, f32(sigma), int(iters), f32(min_parallax), int(min_tri), draws, f1, f2, set(mut), form)


def _initialize(k1, k2, camera, matches12, sigma, iters, min_parallax, min_tri, draws, f1, f2, mut, form):
    n1, n2 = len(k1), len(k2)
    cam6 = [f32(x) for x in camera]
    cam = cam6[:4]
    matches12 = [int(m) if 0 <= int(m) < n2 else -1 for m in matches12]
    prep = prepare(k1, k2, matches12, mut) if sum(1 for m in matches12 if m >= 0) >= 8 else None
    N = sum(1 for m in matches12 if m >= 0)
    info = np.zeros(INFO, np.int32)
    finfo = np.zeros(FINFO, f32)
    info[I_N], info[I_BEST_H], info[I_BEST_F], info[I_CHOSEN] = N, -1, -1, -1
    out = dict(ret=0, trace=[], pose=np.zeros((2, 21), f32), P3D=np.zeros((n1, 3), f32), triangulated=np.zeros(n1, np.uint8),
               matches12_out=np.full(n1, -1, np.int32), info=info, finfo=finfo)
    status = 0
    chosen_res = None
    if N < 8:
        status = FEW                                                      # nothing is evaluated: the trace is zeros
        out["trace"] = [dict(H21=[Z] * 9, F21=[Z] * 9, scoreH=Z, scoreF=Z, inlH=[], inlF=[], set=[0] * 8) for _ in range(iters)]
    else:
        if form == "window":
            tr = window(prep, draws, iters, sigma, mut)
            bH, SH = first_strict_maximum([h["scoreH"] for h in tr], mut)
            bF, SF = first_strict_maximum([h["scoreF"] for h in tr], mut)
        else:
            tr, bH, bF, SH, SF = [], -1, -1, Z, Z
            for it in range(iters):
                h = hypothesis(prep, select_list(draws[it], N), sigma, mut)
                tr.append(h)
                if (h["scoreH"] >= SH and h["scoreH"] > 0) if "best_ge" in mut else h["scoreH"] > SH:
                    bH, SH = it, h["scoreH"]
                if (h["scoreF"] >= SF and h["scoreF"] > 0) if "best_ge" in mut else h["scoreF"] > SF:
                    bF, SF = it, h["scoreF"]
        out["trace"] = tr
        info[I_BEST_H], info[I_BEST_F] = bH, bF
        info[I_INL_H] = sum(tr[bH]["inlH"]) if bH >= 0 else 0
        info[I_INL_F] = sum(tr[bF]["inlF"]) if bF >= 0 else 0
        finfo[F_SH], finfo[F_SF] = SH, SF
        if SH == 0 and SF == 0:
            status = NO_MODEL
        else:
            RH = SH / (SH + SF)
            finfo[F_RH] = RH
            if d(RH) > d(0.40):
                status = MODEL_H
                st, chosen, hyps, res, Nm = reconstruct_h(tr[bH]["H21"], tr[bH]["inlH"], prep, cam, sigma, min_parallax, min_tri, n1, mut)
            else:
                status = MODEL_F
                st, chosen, hyps, res, Nm = reconstruct_f(tr[bF]["F21"], tr[bF]["inlF"], prep, cam, sigma, min_parallax, min_tri, n1, mut)
            status |= st
            info[I_CHOSEN], info[I_MODEL_INL] = chosen, Nm
            for i, r in enumerate(res):
                info[I_NGOOD + i] = r[0]
                finfo[F_PARALLAX + i] = r[1]
            out["cosines"] = [r[4] for r in res]
            if st & OK:
                chosen_res = (hyps[chosen], res[chosen])
    info[I_STATUS] = status
    kf1, kf2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
    pts, of, oi = [], [], []
    if chosen_res:
        (R, t), (_, _, P3D, good, _) = chosen_res
        out["pose"][0] = put_pose(cam6, [ONE, Z, Z, Z, ONE, Z, Z, Z, ONE], [Z, Z, Z])
        out["pose"][1] = put_pose(cam6, R, t)
        for i1, X in P3D.items():
            out["P3D"][i1] = X
        for i1, g in good.items():
            if g:
                out["triangulated"][i1] = 1
        for i1 in range(n1):
            if out["triangulated"][i1]:
                out["matches12_out"][i1] = matches12[i1]
                kf1[i1] = len(pts)
                kf2[matches12[i1]] = len(pts)               # (a keypoint of frame 2 matched twice: the later point keeps the slot)
                pts.append(out["P3D"][i1])
                of += [f1, f2]
                oi += [i1, matches12[i1]]
        out["ret"] = int(out["triangulated"].sum())
        info[I_RET] = out["ret"]
    out.update(points=np.array(pts, f32).reshape(-1, 3), kf_point1=kf1, kf_point2=kf2, obs_start=2 * np.arange(len(pts) + 1, dtype=np.int32),
               obs_frame=np.array(of, np.int32), obs_idx=np.array(oi, np.int32), npoints=len(pts))
    return out
