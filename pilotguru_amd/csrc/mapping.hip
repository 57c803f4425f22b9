// mapping.hip -- LocalMapping::CreateNewMapPoints on gfx950, monocular.
//
// Restates (thirdparty/orb-slam2):
//   LocalMapping::CreateNewMapPoints          src/LocalMapping.cc:209-454
//   LocalMapping::ComputeF12                  src/LocalMapping.cc:538-555
//   MapPoint::UpdateNormalAndDepth            src/MapPoint.cc:347-387
// The pairs are matched by SearchForTriangulation (node_match.hip, through pg_tri_launch) between k_cnm_pairs and k_cnm_triangulate.
#include "match_common.h"

// ---- LocalMapping::CreateNewMapPoints(), monocular (src/LocalMapping.cc:209-454) ----
// Every (key frame, neighbour) pair is matched and triangulated at once, then the first success per KF1 keypoint is kept (the
// equivalence argument is in pgorb.h and DESIGN.md section 4).  Every float operation is written as the reference's cv::Mat
// arithmetic performs it under the readings of OpenCV 2.4.9 recorded in DESIGN.md section 4 (the table of cv::Mat steps):
//   gemm with flags 0 and 3x3 operands: the small-matrix path, float sums, then d = (float)(t*alpha + c*beta) in double;
//   gemm with a transposed operand (R1w*R2w.t()): GEMMSingleMul<float, double>, sums in double;  K1.t().inv()*t12x: a
//   MatOp_Solve, i.e. cv::solve(K1.t(), t12x, DECOMP_LU), float LU with partial pivoting;  K2.inv(): invert's 3x3 closed form
//   in double;  Mat::dot and cv::norm on CV_32F: double;  the rows of A: addWeighted in double;  Mat / double: convertTo
//   with the float scale (float)(1/w);  the SVD: JacobiSVDImpl_<float> on the rows of A^T.
struct PgCnmBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap;
    const pgorb_kf_pose* pose; const uint8_t* hasPoint;
    const int32_t* kf1; const int32_t* neigh; const int32_t* nneigh; int M; const float* median;
    float sf[PG_MAXL + 1];       // mvScaleFactors
    float s2[PG_MAXL + 1];       // mvLevelSigma2
    int nlevels;
    float ratioFactor;           // 1.5f*mfScaleFactor (:233)
};
// per pair: state (0 = searched, PGORB_CNM_SKIPPED = baseline test, -2 = no neighbour in this slot), KF1 / KF2 frames, F12, epipole
struct PgCnmPairs { int32_t* state; int32_t* kf1; int32_t* kf2; float* F12; float* epi; uint8_t* has1; uint8_t* has2; };
struct PgCnmRec { float pos[3], normal[3], minD, maxD; };

// OpenCV's hypot template (lapack.cpp) in double
__device__ __forceinline__ double cnm_hypot(double a, double b)
{
    a = fabs(a); b = fabs(b);
    if (a > b) { b = __ddiv_rn(b, a); return __dmul_rn(a, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(b, b)))); }
    if (b > 0) { a = __ddiv_rn(a, b); return __dmul_rn(b, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(a, a)))); }
    return 0.0;
}

// one thread per pair: the baseline test (:243-262), ComputeF12 (:538-555) and the epipole (ORBmatcher.cc:665-672); then the
// block copies the pair's masks (a skipped or empty pair gets all-set masks, so the matcher finds nothing there)
__global__ __launch_bounds__(256) void k_cnm_pairs(PgCnmBatch B, PgCnmPairs P, float* __restrict__ F12out, float* __restrict__ epiOut)
{
    const int p = blockIdx.x, k = p / B.M, s = p - k * B.M;
    const int f1 = B.kf1[k], nn = min(max(B.nneigh[k], 0), B.M);
    __shared__ int sState, sF2;
    if (threadIdx.x == 0) {
        int state = -2, f2 = f1;
        if (s < nn) {
            f2 = B.neigh[p];
            const pgorb_kf_pose& P1 = B.pose[f1];
            const pgorb_kf_pose& P2 = B.pose[f2];
            const float* T1 = P1.Tcw; const float* T2 = P2.Tcw;
            // baseline = cv::norm(Ow2 - Ow1) (double, to float); ratioBaselineDepth < 0.01 (double)
            const float baseline = cnm_f(cnm_normd(__fsub_rn(P2.Ow[0], P1.Ow[0]), __fsub_rn(P2.Ow[1], P1.Ow[1]), __fsub_rn(P2.Ow[2], P1.Ow[2])));
            state = (double)__fdiv_rn(baseline, B.median[p]) < 0.01 ? PGORB_CNM_SKIPPED : 0;
            // R12 = R1w*R2w.t() (sums in double); t12 = -R1w*R2w.t()*t2w + t1w (the negated product, then the small path with C = t1w)
            float R12[3][3], t12[3];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R12[i][j] = cnm_f(cnm_dotd(T1[4 * i], T1[4 * i + 1], T1[4 * i + 2], T2[4 * j], T2[4 * j + 1], T2[4 * j + 2]));
            for (int i = 0; i < 3; i++) {
                const float t = cnm_dot3f(-R12[i][0], -R12[i][1], -R12[i][2], T2[3], T2[7], T2[11]);
                t12[i] = cnm_f(__dadd_rn((double)t, (double)T1[4 * i + 3]));
            }
            const float S[3][3] = {{0.f, -t12[2], t12[1]}, {t12[2], 0.f, -t12[0]}, {-t12[1], t12[0], 0.f}};   // SkewSymmetricMatrix
            // X = solve(K1.t(), t12x): LUImpl<float> with partial pivoting (a pivot below FLT_EPSILON: solve fails, X = 0)
            float A[3][3] = {{P1.fx, 0.f, 0.f}, {0.f, P1.fy, 0.f}, {P1.cx, P1.cy, 1.f}}, X[3][3];
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) X[i][j] = S[i][j];
            bool ok = true;
            for (int i = 0; i < 3 && ok; i++) {
                int kk = i;
                for (int j = i + 1; j < 3; j++) if (fabsf(A[j][i]) > fabsf(A[kk][i])) kk = j;
                if (fabsf(A[kk][i]) < 1.1920928955078125e-07f) { ok = false; break; }
                if (kk != i) {
                    for (int j = i; j < 3; j++) { const float t = A[i][j]; A[i][j] = A[kk][j]; A[kk][j] = t; }
                    for (int j = 0; j < 3; j++) { const float t = X[i][j]; X[i][j] = X[kk][j]; X[kk][j] = t; }
                }
                const float d = __fdiv_rn(-1.0f, A[i][i]);
                for (int j = i + 1; j < 3; j++) {
                    const float alpha = __fmul_rn(A[j][i], d);
                    for (int c = i + 1; c < 3; c++) A[j][c] = __fadd_rn(A[j][c], __fmul_rn(alpha, A[i][c]));
                    for (int c = 0; c < 3; c++) X[j][c] = __fadd_rn(X[j][c], __fmul_rn(alpha, X[i][c]));
                }
                A[i][i] = -d;
            }
            if (ok) {
                for (int i = 2; i >= 0; i--)
                    for (int j = 0; j < 3; j++) {
                        float sum = X[i][j];
                        for (int c = i + 1; c < 3; c++) sum = __fsub_rn(sum, __fmul_rn(A[i][c], X[c][j]));
                        X[i][j] = __fmul_rn(sum, A[i][i]);
                    }
            } else {
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) X[i][j] = 0.f;
            }
            // Y = X*R12 (small path, + 0.0); K2.inv() (closed form, determinant and cofactors in double); F = Y*K2inv
            float Y[3][3], Ki[3][3], F[3][3];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Y[i][j] = __fadd_rn(cnm_dot3f(X[i][0], X[i][1], X[i][2], R12[0][j], R12[1][j], R12[2][j]), 0.f);
            {
                const float m[3][3] = {{P2.fx, 0.f, P2.cx}, {0.f, P2.fy, P2.cy}, {0.f, 0.f, 1.f}};
#define CNM_M(a, b) ((double)m[a][b])
#define CNM_C(a, b, c, d) __dsub_rn(__dmul_rn(CNM_M(a, b), CNM_M(c, d)), __dmul_rn(CNM_M(a, d), CNM_M(c, b)))
                double det = __dmul_rn(CNM_M(0, 0), CNM_C(1, 1, 2, 2));
                det = __dsub_rn(det, __dmul_rn(CNM_M(0, 1), __dsub_rn(__dmul_rn(CNM_M(1, 0), CNM_M(2, 2)), __dmul_rn(CNM_M(1, 2), CNM_M(2, 0)))));
                det = __dadd_rn(det, __dmul_rn(CNM_M(0, 2), __dsub_rn(__dmul_rn(CNM_M(1, 0), CNM_M(2, 1)), __dmul_rn(CNM_M(1, 1), CNM_M(2, 0)))));
                if (det != 0.0) {
                    const double id = __ddiv_rn(1.0, det);
                    Ki[0][0] = cnm_f(__dmul_rn(CNM_C(1, 1, 2, 2), id)); Ki[0][1] = cnm_f(__dmul_rn(CNM_C(0, 2, 2, 1), id));
                    Ki[0][2] = cnm_f(__dmul_rn(CNM_C(0, 1, 1, 2), id)); Ki[1][0] = cnm_f(__dmul_rn(CNM_C(1, 2, 2, 0), id));
                    Ki[1][1] = cnm_f(__dmul_rn(CNM_C(0, 0, 2, 2), id)); Ki[1][2] = cnm_f(__dmul_rn(CNM_C(0, 2, 1, 0), id));
                    Ki[2][0] = cnm_f(__dmul_rn(CNM_C(1, 0, 2, 1), id)); Ki[2][1] = cnm_f(__dmul_rn(CNM_C(0, 1, 2, 0), id));
                    Ki[2][2] = cnm_f(__dmul_rn(CNM_C(0, 0, 1, 1), id));
                } else {
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ki[i][j] = 0.f;
                }
#undef CNM_C
#undef CNM_M
            }
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) F[i][j] = __fadd_rn(cnm_dot3f(Y[i][0], Y[i][1], Y[i][2], Ki[0][j], Ki[1][j], Ki[2][j]), 0.f);
            // the epipole: C2 = R2w*Cw + t2w (small path with C), invz = 1.0f/C2.z, ex = fx*C2.x*invz + cx (float)
            float C2[3];
            for (int i = 0; i < 3; i++)
                C2[i] = cnm_f(__dadd_rn((double)cnm_dot3f(T2[4 * i], T2[4 * i + 1], T2[4 * i + 2], P1.Ow[0], P1.Ow[1], P1.Ow[2]), (double)T2[4 * i + 3]));
            const float invz = __fdiv_rn(1.0f, C2[2]);
            const float ex = __fadd_rn(__fmul_rn(__fmul_rn(P2.fx, C2[0]), invz), P2.cx);
            const float ey = __fadd_rn(__fmul_rn(__fmul_rn(P2.fy, C2[1]), invz), P2.cy);
            for (int i = 0; i < 9; i++) { P.F12[(int64_t)p * 9 + i] = F[i / 3][i % 3]; if (F12out) F12out[(int64_t)p * 9 + i] = F[i / 3][i % 3]; }
            P.epi[2 * p] = ex; P.epi[2 * p + 1] = ey;
            if (epiOut) { epiOut[2 * p] = ex; epiOut[2 * p + 1] = ey; }
        } else {
            for (int i = 0; i < 9; i++) { P.F12[(int64_t)p * 9 + i] = 0.f; if (F12out) F12out[(int64_t)p * 9 + i] = 0.f; }
            P.epi[2 * p] = P.epi[2 * p + 1] = 0.f;
            if (epiOut) epiOut[2 * p] = epiOut[2 * p + 1] = 0.f;
        }
        P.state[p] = state; P.kf1[p] = f1; P.kf2[p] = f2;
        sState = state; sF2 = f2;
    }
    __syncthreads();
    const int state = sState, f2 = sF2, cap = B.cap;
    uint8_t* h1 = P.has1 + (int64_t)p * cap; uint8_t* h2 = P.has2 + (int64_t)p * cap;
    const uint8_t* e1 = B.hasPoint ? B.hasPoint + (int64_t)f1 * cap : nullptr;
    const uint8_t* e2 = B.hasPoint ? B.hasPoint + (int64_t)f2 * cap : nullptr;
    for (int i = threadIdx.x; i < cap; i += 256) {
        h1[i] = state ? 1 : (e1 ? e1[i] : 0);
        h2[i] = state ? 1 : (e2 ? e2[i] : 0);
    }
}

// JacobiSVDImpl_<float> (lapack.cpp) on a 4x4: At = A^T (its rows are A's columns), W the squared row norms in double, cyclic
// sweeps (at most 30) until one rotates nothing, then W = sqrt of the row norms, a selection sort to descending W that swaps
// Vt's rows.  Returns Vt's row 3.
__device__ __forceinline__ void cnm_svd_v3(float At[4][4], float v3[4])
{
    float Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd = __dadd_rn(sd, __dmul_rn((double)At[i][k], (double)At[i][k]));
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < 4; k++) Vt[i][k] = i == k ? 1.f : 0.f;
    }
    const float eps = 2.3841857910156250e-07f;                    // FLT_EPSILON*2
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                const double a = W[i], b = W[j];
                double p = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) p = __dadd_rn(p, __dmul_rn((double)At[i][k], (double)At[j][k]));
                if (fabs(p) <= __dmul_rn((double)eps, __dsqrt_rn(__dmul_rn(a, b)))) continue;
                p = __dmul_rn(p, 2.0);
                const double beta = __dsub_rn(a, b), gamma = cnm_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = __dmul_rn(__dsub_rn(gamma, beta), 0.5);
                    s = cnm_f(__dsqrt_rn(__ddiv_rn(delta, gamma)));
                    c = cnm_f(__ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, (double)s), 2.0)));
                } else {
                    c = cnm_f(__dsqrt_rn(__ddiv_rn(__dadd_rn(gamma, beta), __dmul_rn(gamma, 2.0))));
                    s = cnm_f(__ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, (double)c), 2.0)));
                }
                double na = 0.0, nb = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = __fadd_rn(__fmul_rn(c, At[i][k]), __fmul_rn(s, At[j][k]));
                    const float t1 = __fadd_rn(__fmul_rn(-s, At[i][k]), __fmul_rn(c, At[j][k]));
                    At[i][k] = t0; At[j][k] = t1;
                    na = __dadd_rn(na, __dmul_rn((double)t0, (double)t0)); nb = __dadd_rn(nb, __dmul_rn((double)t1, (double)t1));
                }
                W[i] = na; W[j] = nb;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = __fadd_rn(__fmul_rn(c, Vt[i][k]), __fmul_rn(s, Vt[j][k]));
                    const float t1 = __fadd_rn(__fmul_rn(-s, Vt[i][k]), __fmul_rn(c, Vt[j][k]));
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) sd = __dadd_rn(sd, __dmul_rn((double)At[i][k], (double)At[i][k]));
        W[i] = __dsqrt_rn(sd);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 4; k++) if (W[j] < W[k]) j = k;
        if (j != i) {
            // (only the rows that end at 3 matter; the swap is written out with constant indices to keep Vt in registers)
#pragma unroll
            for (int jj = i + 1; jj < 4; jj++)
                if (jj == j) {
                    const double tw = W[i]; W[i] = W[jj]; W[jj] = tw;
#pragma unroll
                    for (int k = 0; k < 4; k++) { const float t = Vt[i][k]; Vt[i][k] = Vt[jj][k]; Vt[jj][k] = t; }
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) v3[k] = Vt[3][k];
}

// one lane per (pair, KF1 keypoint) with a match: the triangulation and its tests (:282-423); a failure clears the match
__global__ __launch_bounds__(64) void k_cnm_triangulate(PgCnmBatch B, const int32_t* __restrict__ pairKF1, const int32_t* __restrict__ pairKF2,
                                                        int32_t* __restrict__ matches, PgCnmRec* __restrict__ rec)
{
    const int p = blockIdx.y, idx1 = blockIdx.x * 64 + threadIdx.x, cap = B.cap;
    const int f1 = pairKF1[p], f2 = pairKF2[p];
    if (idx1 >= min(B.n[f1], cap)) return;
    int32_t* mp = matches + (int64_t)p * cap + idx1;
    const int idx2 = *mp;
    if (idx2 < 0) return;
    const pgorb_kf_pose& P1 = B.pose[f1];
    const pgorb_kf_pose& P2 = B.pose[f2];
    const float* T1 = P1.Tcw; const float* T2 = P2.Tcw;
    const pgorb_keypoint kp1 = B.K[(int64_t)f1 * cap + idx1], kp2 = B.K[(int64_t)f2 * cap + idx2];
    bool ok = false;
    PgCnmRec r;
    do {
        // xn = ((x - cx)*invfx, (y - cy)*invfy, 1); ray = Rwc*xn (small path); cosParallaxRays = dot/(norm*norm) in double, to float
        const float xa = __fmul_rn(__fsub_rn(kp1.x, P1.cx), P1.invfx), ya = __fmul_rn(__fsub_rn(kp1.y, P1.cy), P1.invfy);
        const float xb = __fmul_rn(__fsub_rn(kp2.x, P2.cx), P2.invfx), yb = __fmul_rn(__fsub_rn(kp2.y, P2.cy), P2.invfy);
        float r1[3], r2[3];
        for (int i = 0; i < 3; i++) {
            r1[i] = __fadd_rn(cnm_dot3f(T1[i], T1[4 + i], T1[8 + i], xa, ya, 1.f), 0.f);
            r2[i] = __fadd_rn(cnm_dot3f(T2[i], T2[4 + i], T2[8 + i], xb, yb, 1.f), 0.f);
        }
        const float cosPar = cnm_f(__ddiv_rn(cnm_dotd(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]),
                                             __dmul_rn(cnm_normd(r1[0], r1[1], r1[2]), cnm_normd(r2[0], r2[1], r2[2]))));
        const float cosStereo = __fadd_rn(cosPar, 1.f);
        if (!(cosPar < cosStereo && cosPar > 0 && (double)cosPar < 0.9998)) break;
        // A (4x4): rows xn*Tcw.row(2) - Tcw.row(r) by addWeighted in double; At = A^T
        float At[4][4];
        for (int c = 0; c < 4; c++) {
            At[c][0] = cnm_f(__dadd_rn(__dadd_rn(__dmul_rn((double)T1[8 + c], (double)xa), -(double)T1[c]), 0.0));
            At[c][1] = cnm_f(__dadd_rn(__dadd_rn(__dmul_rn((double)T1[8 + c], (double)ya), -(double)T1[4 + c]), 0.0));
            At[c][2] = cnm_f(__dadd_rn(__dadd_rn(__dmul_rn((double)T2[8 + c], (double)xb), -(double)T2[c]), 0.0));
            At[c][3] = cnm_f(__dadd_rn(__dadd_rn(__dmul_rn((double)T2[8 + c], (double)yb), -(double)T2[4 + c]), 0.0));
        }
        float v[4];
        cnm_svd_v3(At, v);
        if (v[3] == 0.f) break;
        const float sc = cnm_f(__ddiv_rn(1.0, (double)v[3]));       // x3D.rowRange(0,3)/w: convertTo with the float scale
        const float X0 = __fadd_rn(__fmul_rn(v[0], sc), 0.f), X1 = __fadd_rn(__fmul_rn(v[1], sc), 0.f), X2 = __fadd_rn(__fmul_rn(v[2], sc), 0.f);
        // z = Rcw.row(2).dot(x3D) + t (double, to float)
        const float z1 = cnm_f(__dadd_rn(cnm_dotd(T1[8], T1[9], T1[10], X0, X1, X2), (double)T1[11]));
        if (z1 <= 0) break;
        const float z2 = cnm_f(__dadd_rn(cnm_dotd(T2[8], T2[9], T2[10], X0, X1, X2), (double)T2[11]));
        if (z2 <= 0) break;
        const int o1 = min((unsigned)kp1.octave, (unsigned)PG_MAXL), o2 = min((unsigned)kp2.octave, (unsigned)PG_MAXL);
        {
            const float x1 = cnm_f(__dadd_rn(cnm_dotd(T1[0], T1[1], T1[2], X0, X1, X2), (double)T1[3]));
            const float y1 = cnm_f(__dadd_rn(cnm_dotd(T1[4], T1[5], T1[6], X0, X1, X2), (double)T1[7]));
            const float invz1 = cnm_f(__ddiv_rn(1.0, (double)z1));
            const float u1 = __fadd_rn(__fmul_rn(__fmul_rn(P1.fx, x1), invz1), P1.cx), v1 = __fadd_rn(__fmul_rn(__fmul_rn(P1.fy, y1), invz1), P1.cy);
            const float ex = __fsub_rn(u1, kp1.x), ey = __fsub_rn(v1, kp1.y);
            if ((double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > __dmul_rn(5.991, (double)B.s2[o1])) break;
        }
        {
            const float x2 = cnm_f(__dadd_rn(cnm_dotd(T2[0], T2[1], T2[2], X0, X1, X2), (double)T2[3]));
            const float y2 = cnm_f(__dadd_rn(cnm_dotd(T2[4], T2[5], T2[6], X0, X1, X2), (double)T2[7]));
            const float invz2 = cnm_f(__ddiv_rn(1.0, (double)z2));
            const float u2 = __fadd_rn(__fmul_rn(__fmul_rn(P2.fx, x2), invz2), P2.cx), v2 = __fadd_rn(__fmul_rn(__fmul_rn(P2.fy, y2), invz2), P2.cy);
            const float ex = __fsub_rn(u2, kp2.x), ey = __fsub_rn(v2, kp2.y);
            if ((double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > __dmul_rn(5.991, (double)B.s2[o2])) break;
        }
        // scale consistency (:397-413)
        const float n1x = __fsub_rn(X0, P1.Ow[0]), n1y = __fsub_rn(X1, P1.Ow[1]), n1z = __fsub_rn(X2, P1.Ow[2]);
        const float n2x = __fsub_rn(X0, P2.Ow[0]), n2y = __fsub_rn(X1, P2.Ow[1]), n2z = __fsub_rn(X2, P2.Ow[2]);
        const double d1d = cnm_normd(n1x, n1y, n1z), d2d = cnm_normd(n2x, n2y, n2z);
        const float dist1 = cnm_f(d1d), dist2 = cnm_f(d2d);
        if (dist1 == 0 || dist2 == 0) break;
        const float ratioDist = __fdiv_rn(dist2, dist1), ratioOctave = __fdiv_rn(B.sf[o1], B.sf[o2]);
        if (__fmul_rn(ratioDist, B.ratioFactor) < ratioOctave || ratioDist > __fmul_rn(ratioOctave, B.ratioFactor)) break;
        // UpdateNormalAndDepth: normal = sum of normali*(float)(1/norm) over the two observations, then /2; dist = dist1 (KF1 is
        // the reference key frame); mfMaxDistance = dist*mvScaleFactors[octave1], mfMinDistance = mfMaxDistance/mvScaleFactors[nlevels-1]
        const float s1 = cnm_f(__ddiv_rn(1.0, d1d)), s2 = cnm_f(__ddiv_rn(1.0, d2d));
        r.pos[0] = X0; r.pos[1] = X1; r.pos[2] = X2;
        r.normal[0] = __fmul_rn(__fadd_rn(__fmul_rn(n1x, s1), __fmul_rn(n2x, s2)), 0.5f);
        r.normal[1] = __fmul_rn(__fadd_rn(__fmul_rn(n1y, s1), __fmul_rn(n2y, s2)), 0.5f);
        r.normal[2] = __fmul_rn(__fadd_rn(__fmul_rn(n1z, s1), __fmul_rn(n2z, s2)), 0.5f);
        r.maxD = __fmul_rn(dist1, B.sf[o1]);
        r.minD = __fdiv_rn(r.maxD, B.sf[max(B.nlevels - 1, 0)]);
        ok = true;
    } while (false);
    if (ok) rec[(int64_t)p * cap + idx1] = r;
    else *mp = -1;
}

// one workgroup per current key frame: the first neighbour whose match of idx1 triangulated wins; the points in the reference's
// creation order (neighbour, then ascending idx1): one wave per neighbour slot ranks its winners with ballots
#define CNM_T 1024
__global__ __launch_bounds__(CNM_T) void k_cnm_resolve(PgCnmBatch B, const int32_t* __restrict__ state, const int32_t* __restrict__ matches,
                                                       const PgCnmRec* __restrict__ rec, pgorb_new_map_point* __restrict__ points,
                                                       int32_t* __restrict__ npoints, int32_t* __restrict__ count, uint8_t* __restrict__ has1out)
{
    __shared__ int8_t win[16000];
    __shared__ int cnt[PGORB_CNM_MAX_NEIGHBOURS], off[PGORB_CNM_MAX_NEIGHBOURS];
    const int k = blockIdx.x, tid = threadIdx.x, cap = B.cap, M = B.M;
    const int f1 = B.kf1[k], n1 = min(B.n[f1], cap), nn = min(max(B.nneigh[k], 0), M);
    if (tid < PGORB_CNM_MAX_NEIGHBOURS) cnt[tid] = 0;
    __syncthreads();
    const uint8_t* e1 = B.hasPoint ? B.hasPoint + (int64_t)f1 * cap : nullptr;
    for (int i = tid; i < cap; i += CNM_T) {
        int w = -1;
        if (i < n1) {
            for (int s = 0; s < nn; s++)
                if (matches[((int64_t)k * M + s) * cap + i] >= 0) { w = s; break; }
            win[i] = (int8_t)w;
            if (w >= 0) atomicAdd(&cnt[w], 1);
        }
        if (has1out) has1out[(int64_t)k * cap + i] = (uint8_t)((e1 && e1[i]) || w >= 0);
    }
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int s = 0; s < nn; s++) { off[s] = t; t += cnt[s]; }
        npoints[k] = t;
    }
    if (tid < M) count[(int64_t)k * M + tid] = tid >= nn ? 0 : (state[k * M + tid] == PGORB_CNM_SKIPPED ? PGORB_CNM_SKIPPED : cnt[tid]);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int s = wave; s < nn; s += CNM_T / 64) {
        int base = off[s];
        const int64_t p = (int64_t)k * M + s;
        for (int c0 = 0; c0 < n1; c0 += 64) {
            const int i = c0 + lane;
            const bool hit = i < n1 && win[i] == s;
            const unsigned long long bal = __ballot(hit);
            if (hit) {
                const PgCnmRec& r = rec[p * cap + i];
                pgorb_new_map_point o;
                o.neighbour = s; o.idx1 = i; o.idx2 = matches[p * cap + i];
                for (int q = 0; q < 3; q++) { o.pos[q] = r.pos[q]; o.normal[q] = r.normal[q]; }
                o.min_distance = r.minD; o.max_distance = r.maxD;
                points[(int64_t)k * cap + base + __popcll(bal & ((1ull << lane) - 1ull))] = o;
            }
            base += __popcll(bal);
        }
    }
}

extern "C" {

// one key frame through host buffers: KF1 = frame 0, neighbour s = frame s + 1 of one batch
int pgorb_create_new_map_points(pgorb_ctx* c, const pgorb_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_point1, int n1,
                                const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1, const pgorb_kf_pose* pose1,
                                int nneigh, const pgorb_keypoint* const* kps2, const uint8_t* const* desc2, const uint8_t* const* has_point2,
                                const int32_t* n2, const uint32_t* const* fv2_node, const int32_t* const* fv2_start, const uint32_t* const* fv2_feat,
                                const int32_t* nfv2, const pgorb_kf_pose* pose2, const float* median_depth2, pgorb_new_map_point* points,
                                int32_t* count, float* F12, float* epipole, uint8_t* has_point1_out)
{
    if (!c) return PGORB_E_ARG;
    const char* bad = "bad argument to pgorb_create_new_map_points";
    if (n1 < 0 || nfv1 < 0 || nneigh < 0 || !pose1 || !fv1_start || (nfv1 && (!fv1_node || !fv1_feat)) || (n1 && (!kps1 || !desc1 || !points)) ||
        (nneigh && (!kps2 || !desc2 || !n2 || !fv2_node || !fv2_start || !fv2_feat || !nfv2 || !pose2 || !median_depth2 || !count)))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (nneigh > PGORB_CNM_MAX_NEIGHBOURS) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 64 neighbours per key frame");
    if (n1 > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (!pg_fv_ok(fv1_start, fv1_feat, nfv1, n1))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_create_new_map_points: FeatureVector names more features than the key frame has");
    std::vector<PgFvFrame> f(nneigh + 1);
    f[0] = {kps1, nullptr, desc1, has_point1, n1, fv1_node, fv1_start, fv1_feat, nfv1};
    for (int s = 0; s < nneigh; s++) {
        const int n = n2[s], m = nfv2[s];
        if (n < 0 || m < 0 || !fv2_start[s] || (n && (!kps2[s] || !desc2[s])) || (m && (!fv2_node[s] || !fv2_feat[s])))
            return pg_ctx_fail(c, PGORB_E_ARG, bad);
        if (n > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        if (!pg_fv_ok(fv2_start[s], fv2_feat[s], m, n))
            return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_create_new_map_points: FeatureVector names more features than the key frame has");
        f[s + 1] = {kps2[s], nullptr, desc2[s], has_point2 ? has_point2[s] : nullptr, n, fv2_node[s], fv2_start[s], fv2_feat[s], m};
    }
    for (int s = 0; s < nneigh; s++) count[s] = 0;
    if (has_point1_out) for (int i = 0; i < n1; i++) has_point1_out[i] = has_point1 ? (has_point1[i] != 0) : 0;
    if (F12) memset(F12, 0, (size_t)nneigh * 36);
    if (epipole) memset(epipole, 0, (size_t)nneigh * 8);
    if (!nneigh) return 0;
    PgHostCall hc(c);
    const PgFvPack fp(hc, f.data(), nneigh + 1);                  // kf1 = fp.P[0], the neighbours fp.P[1 ..]
    const int cap = fp.cap;
    const size_t PO = hc.region(PG_UP, (nneigh + 1) * sizeof(pgorb_kf_pose)), NN = hc.region(PG_UP, 4), MD = hc.region(PG_UP, nneigh * 4),
                 oP = hc.region(PG_DOWN, (size_t)cap * sizeof(pgorb_new_map_point)), oNP = hc.region(PG_DOWN, 4), oC = hc.region(PG_DOWN, nneigh * 4),
                 oF = hc.region(PG_DOWN, nneigh * 36), oE = hc.region(PG_DOWN, nneigh * 8), oH = hc.region(PG_DOWN, cap);
    int rc = hc.begin();
    if (rc) return rc;
    fp.pack(hc, f.data());
    for (int k = 0; k <= nneigh; k++) hc.host<pgorb_kf_pose>(PO)[k] = k ? pose2[k - 1] : *pose1;
    *hc.host<int32_t>(NN) = nneigh;
    hc.put(MD, median_depth2, nneigh * 4);
    if ((rc = hc.run([&] {
            return pgorb_create_new_map_points_batch_device(c, hc.dev<pgorb_keypoint>(fp.K), hc.dev(fp.D), hc.dev<int32_t>(fp.N), cap, hc.dev<uint32_t>(fp.FN),
                                                            hc.dev<int32_t>(fp.FS), hc.dev<uint32_t>(fp.FF), hc.dev<int32_t>(fp.NF), hc.dev<pgorb_kf_pose>(PO),
                                                            hc.dev(fp.H), hc.dev<int32_t>(fp.P), 1, hc.dev<int32_t>(fp.P) + 1, hc.dev<int32_t>(NN), nneigh,
                                                            hc.dev<float>(MD), hc.dev<pgorb_new_map_point>(oP), hc.dev<int32_t>(oNP),
                                                            hc.dev<int32_t>(oC), hc.dev<float>(oF), hc.dev<float>(oE), hc.dev(oH), nullptr); }))) return rc;
    const int np = *hc.host<int32_t>(oNP);
    memcpy(points, hc.host(oP), (size_t)np * sizeof(pgorb_new_map_point));
    memcpy(count, hc.host(oC), (size_t)nneigh * 4);
    if (F12) memcpy(F12, hc.host(oF), (size_t)nneigh * 36);
    if (epipole) memcpy(epipole, hc.host(oE), (size_t)nneigh * 8);
    if (has_point1_out) memcpy(has_point1_out, hc.host(oH), (size_t)n1);
    return np;
}

int pgorb_create_new_map_points_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                             const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
                                             const pgorb_kf_pose* d_pose, const uint8_t* d_has_point, const int32_t* d_kf1, int nkf,
                                             const int32_t* d_neigh, const int32_t* d_nneigh, int max_neigh, const float* d_median_depth,
                                             pgorb_new_map_point* d_points, int32_t* d_npoints, int32_t* d_count, float* d_F12, float* d_epipole,
                                             uint8_t* d_has_point1_out, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv || nkf < 0 || max_neigh < 1 ||
        (nkf && (!d_pose || !d_kf1 || !d_neigh || !d_nneigh || !d_median_depth || !d_points || !d_npoints || !d_count)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_create_new_map_points_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (max_neigh > PGORB_CNM_MAX_NEIGHBOURS) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 64 neighbours per key frame");
    if (!nkf) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const size_t npairs = (size_t)nkf * max_neigh, pc = npairs * cap;
    // one scratch arena: matches, triangulated points, bins, both masks, then the pair tables
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t oM = take(pc * 4), oR = take(pc * sizeof(PgCnmRec)), oB = take(pc), oH1 = take(pc), oH2 = take(pc), oNM = take(npairs * 4),
                 oS = take(npairs * 4), oK1 = take(npairs * 4), oK2 = take(npairs * 4), oF = take(npairs * 36), oE = take(npairs * 8);
    void* scr;
    int rc = pg_ctx_scratch(c, o, s, &scr);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)scr;
    const PgCnmPairs P = {(int32_t*)(base + oS), (int32_t*)(base + oK1), (int32_t*)(base + oK2), (float*)(base + oF), (float*)(base + oE),
                          base + oH1, base + oH2};
    PgCnmBatch B = {d_kps, d_n, cap, d_pose, d_has_point, d_kf1, d_neigh, d_nneigh, max_neigh, d_median_depth, {0}, {0}, 0, 0.f};
    pgorb_scale_tables(c, B.sf, nullptr, B.s2, nullptr);
    B.nlevels = pgorb_levels(c);
    B.ratioFactor = 1.5f * B.sf[1];                               // mfScaleFactor = mvScaleFactors[1] (ORBextractor.cc:414-418)
    hipLaunchKernelGGL(k_cnm_pairs, dim3((unsigned)npairs), dim3(256), 0, s, B, P, d_F12, d_epipole);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cnm_pairs launch failed");
    const PgTriBatch T = {{d_kps, d_desc, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv}, P.kf1, P.kf2, P.F12, P.epi, P.has2, {0}, {0}};
    if ((rc = pg_tri_launch(c, T, (int)npairs, P.has1, 0, (int32_t*)(base + oM), (int8_t*)(base + oB), (int32_t*)(base + oNM), s)))
        return rc;
    hipLaunchKernelGGL(k_cnm_triangulate, dim3((unsigned)((cap + 63) / 64), (unsigned)npairs), dim3(64), 0, s, B, (const int32_t*)P.kf1,
                       (const int32_t*)P.kf2, (int32_t*)(base + oM), (PgCnmRec*)(base + oR));
    hipLaunchKernelGGL(k_cnm_resolve, dim3((unsigned)nkf), dim3(CNM_T), 0, s, B, (const int32_t*)P.state, (const int32_t*)(base + oM),
                       (const PgCnmRec*)(base + oR), d_points, d_npoints, d_count, d_has_point1_out);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cnm_triangulate launch failed");
    return pg_ctx_scratch_done(c, s);
}

}  // extern "C"
