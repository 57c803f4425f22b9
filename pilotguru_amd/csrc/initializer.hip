// initializer.hip -- Initializer on gfx950: the two-view homography / fundamental RANSAC that starts a monocular map, every
// hypothesis of the call evaluated at once and the reference's sequential best-update applied afterwards, then the motion
// hypotheses of the chosen model reconstructed and the map of Tracking::CreateInitialMapMonocular laid out.
//
// Restates (thirdparty/orb-slam2):
//   Initializer::Initialize                       src/Initializer.cc:44-121 (the matches compacted in i1 order, the sets)
//   FindHomography / FindFundamental              :124-223 (the first strict maximum of the score above 0)
//   ComputeH21 / ComputeF21                       :226-303 (jacobi_f32.h; vt.row(8) of the 8 x 9 system is the completion vector)
//   CheckHomography / CheckFundamental            :305-468 (float throughout, ONE sequential sum)
//   ReconstructF / ReconstructH / DecomposeE      :470-732, :909-929
//   Triangulate / Normalize / CheckRT             :734-907
//   DUtils::Random::RandomInt                     DUtils/Random.cpp:47-50
//   Tracking::MonocularInitialization             src/Tracking.cc:610-626 (matches12_out, the two poses)
//   Tracking::CreateInitialMapMonocular           src/Tracking.cc:633-680 (the points, the slots and the observations)
// under the readings of DESIGN.md section 4 (the Initializer rows); tests/init_reference.py is the definition.
//
// Three launches per call, none with atomics:
//   k_init_prepare      one workgroup per pair: Normalize over ALL keypoints of both frames (one lane does the ordered sums over
//                       chunks staged in LDS), T1, T2inv, T2t, and the matches compacted in i1 order by ballot prefix.
//   k_init_hypotheses   one wave per (pair, iteration, model): the set from the caller's draws, the Jacobi with its matrices in
//                       LDS, then the lanes stride over the N matches; the score is folded lane by lane in index order, the
//                       count is a sum of ballot popcounts and the ballots themselves are the inlier mask.
//   k_init_reconstruct  one workgroup per pair: the best hypothesis of each model, RH and the branch, the 8 or 4 motion
//                       hypotheses, CheckRT with the threads spread over (hypothesis, match), the order statistic of the
//                       parallax by a radix search, the decision and every remaining output.
#include "match_common.h"
#include "jacobi_f32.h"
#include <math.h>
#include <string>

#define INIT_T 256
#define INIT_WAVES (INIT_T / 64)
#define INIT_MAX_N 16000
#define INIT_CHUNK 2048
#define IN_HD __device__ __forceinline__

static_assert(sizeof(pgorb_init_hypothesis) == 120, "18 floats, 2 floats, 10 int32");
static_assert(sizeof(pgorb_kf_pose) == 84, "21 floats");

// ---- the cv::Mat steps ----
IN_HD float in_dot3(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return jf_add(jf_add(jf_mul(a0, b0), jf_mul(a1, b1)), jf_mul(a2, b2));
}
// gemm's small-matrix epilogue (float)(t*alpha + c*beta) in double: without C a + 0.0, which turns a -0 sum into +0
IN_HD float in_small(float t) { return jd_f(jd_add((double)t, 0.0)); }
IN_HD float in_small_alpha(float t, float alpha) { return jd_f(jd_add(jd_mul((double)t, (double)alpha), 0.0)); }
IN_HD float in_small_c(float t, float c) { return jd_f(jd_add((double)t, (double)c)); }
IN_HD void in_mul33(const float* A, const float* B, float* D)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[3 * i + j] = in_small(in_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]));
}
IN_HD void in_mul33_alpha(const float* A, const float* B, float alpha, float* D)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) D[3 * i + j] = in_small_alpha(in_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]), alpha);
}
// a transposed operand: GEMMSingleMul<float, double>, sums in double from 0, rounded once.  ta: A.t()*B; else A*B.t()
IN_HD void in_mul33_t(const float* A, const float* B, bool ta, float* D)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) s = jd_add(s, jd_mul((double)(ta ? A[3 * k + i] : A[3 * i + k]), (double)(ta ? B[3 * k + j] : B[3 * j + k])));
            D[3 * i + j] = jd_f(s);
        }
}
// cv::invert's 3 x 3 closed form: determinant and cofactors in double; det == 0 gives the zero matrix
IN_HD void in_inv33(const float* M, float* D)
{
#define IN_C(a, b, c, e) jd_sub(jd_mul((double)M[a], (double)M[b]), jd_mul((double)M[c], (double)M[e]))
    double det = jd_mul((double)M[0], IN_C(4, 8, 5, 7));
    det = jd_sub(det, jd_mul((double)M[1], IN_C(3, 8, 5, 6)));
    det = jd_add(det, jd_mul((double)M[2], IN_C(3, 7, 4, 6)));
    if (det != 0.0) {
        const double id = jd_div(1.0, det);
        D[0] = jd_f(jd_mul(IN_C(4, 8, 5, 7), id)); D[1] = jd_f(jd_mul(IN_C(2, 7, 1, 8), id)); D[2] = jd_f(jd_mul(IN_C(1, 5, 2, 4), id));
        D[3] = jd_f(jd_mul(IN_C(5, 6, 3, 8), id)); D[4] = jd_f(jd_mul(IN_C(0, 8, 2, 6), id)); D[5] = jd_f(jd_mul(IN_C(2, 3, 0, 5), id));
        D[6] = jd_f(jd_mul(IN_C(3, 7, 4, 6), id)); D[7] = jd_f(jd_mul(IN_C(1, 6, 0, 7), id)); D[8] = jd_f(jd_mul(IN_C(0, 4, 1, 3), id));
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) D[i] = 0.f;
    }
#undef IN_C
}
// cv::determinant of a 3 x 3 CV_32F: det3 in float, widened
IN_HD double in_det33(const float* m)
{
    const float a = jf_mul(m[0], jf_sub(jf_mul(m[4], m[8]), jf_mul(m[5], m[7])));
    const float b = jf_mul(m[1], jf_sub(jf_mul(m[3], m[8]), jf_mul(m[5], m[6])));
    const float c = jf_mul(m[2], jf_sub(jf_mul(m[3], m[7]), jf_mul(m[4], m[6])));
    return (double)jf_add(jf_sub(a, b), c);
}
IN_HD double in_dotd(const float* a, const float* b)
{
    double s = jd_add(0.0, jd_mul((double)a[0], (double)b[0]));
    s = jd_add(s, jd_mul((double)a[1], (double)b[1]));
    return jd_add(s, jd_mul((double)a[2], (double)b[2]));
}
IN_HD double in_normd(const float* a) { return jd_sqrt(in_dotd(a, a)); }
// Mat / double and Mat *= double: convertTo with the float scale, x*(float)s + 0
IN_HD void in_scale3(float* v, double s)
{
    const float f = jd_f(s);
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = jf_add(jf_mul(v[i], f), 0.f);
}

// cv::SVD::compute of a 3 x 3 (m = n: the Jacobi on the rows of M^T, then the completion).  wsA, wsV [9*S], wsW [3*S]: the workspace.
template <int S>
IN_HD void in_svd33(const float* M, float* wsA, float* wsV, double* wsW, float* w, float* U, float* Vt)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) wsA[(3 * i + k) * S] = M[3 * k + i];
    jf_jacobi<3, 3, S>(wsA, wsV, wsW);
    jf_complete<3, 3, 3, S>(wsA, wsW);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) { U[3 * r + c] = wsA[(3 * c + r) * S]; Vt[3 * r + c] = wsV[(3 * r + c) * S]; }
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = jd_f(wsW[i * S]);
}

// ---- the hypotheses ----
// DUtils::Random::RandomInt(0, size - 1) of a raw rand() value
IN_HD int in_random_int(uint32_t r, int size) { return (int)(((double)r / 2147483648.0) * (double)size); }
// the indices of :84-96 without the list (as pnp_select): only the positions a swap has overwritten are kept
IN_HD void in_select8(const uint32_t* d, int N, int* out)
{
    int pos[8], val[8];
    int size = N;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        int r = in_random_int(d[j], size);
        r = r < 0 ? 0 : (r > size - 1 ? size - 1 : r);                // (a draw >= 2^31 in the unchecked form)
        int pick = r, back = size - 1;
#pragma unroll
        for (int a = 0; a < j; a++) { if (pos[a] == r) pick = val[a]; if (pos[a] == size - 1) back = val[a]; }
        out[j] = pick;
        pos[j] = r; val[j] = back;
        size--;
    }
}

// the two rows of ComputeH21's A for correspondence j, as columns 2j and 2j+1 of At (9 rows of 16)
IN_HD void in_h_rows(float* At, int j, float u1, float v1, float u2, float v2)
{
    const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, jf_mul(v2, u1), jf_mul(v2, v1), v2};
    const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, jf_mul(-u2, u1), jf_mul(-u2, v1), -u2};
#pragma unroll
    for (int c = 0; c < 9; c++) { At[c * 16 + 2 * j] = r0[c]; At[c * 16 + 2 * j + 1] = r1[c]; }
}
// the row of ComputeF21's A (8 rows of 9; a ninth row follows for the completion)
IN_HD void in_f_row(float* A, int j, float u1, float v1, float u2, float v2)
{
    float* r = A + 9 * j;
    r[0] = jf_mul(u2, u1); r[1] = jf_mul(u2, v1); r[2] = u2; r[3] = jf_mul(v2, u1); r[4] = jf_mul(v2, v1); r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1.f;
}
// H21i = T2inv*Hn*T1 and H12i = H21i.inv() from the filled At; wsV [81], wsW [9]
IN_HD void in_solve_h(float* At, float* wsV, double* wsW, const float* T1, const float* T2inv, float* H21, float* H12)
{
    jf_jacobi<9, 16, 1>(At, wsV, wsW);
    float Hn[9], X[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Hn[i] = wsV[72 + i];
    in_mul33(T2inv, Hn, X);
    in_mul33(X, T1, H21);
    in_inv33(H21, H12);
}
// F21i = T2t*Fn*T1 from the filled A (room for 9 rows of 9); ws3A, ws3V [9], wsW [9]
IN_HD void in_solve_f(float* A, float* ws3A, float* ws3V, double* wsW, const float* T1, const float* T2t, float* F21)
{
    jf_jacobi<8, 9, 1>(A, nullptr, wsW);
    jf_complete<8, 9, 9, 1>(A, wsW);
    float pre[9], w[3], U[9], Vt[9], X[9], Fn[9];
#pragma unroll
    for (int i = 0; i < 9; i++) pre[i] = A[72 + i];
    in_svd33<1>(pre, ws3A, ws3V, wsW, w, U, Vt);
    const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, 0.f};
    in_mul33(U, D, X);
    in_mul33(X, Vt, Fn);
    in_mul33(T2t, Fn, X);
    in_mul33(X, T1, F21);
}

#define IN_TH 5.991f
#define IN_TH_F 3.841f
// the two terms of one match under CheckHomography (:337-385): 0 for a term that is not added; in = bIn
IN_HD void in_check_h(const float* h, const float* g, float u1, float v1, float u2, float v2, float invS2, float& t1, float& t2, bool& in)
{
    float w = jd_f(jd_div(1.0, (double)jf_add(jf_add(jf_mul(g[6], u2), jf_mul(g[7], v2)), g[8])));
    float a = jf_mul(jf_add(jf_add(jf_mul(g[0], u2), jf_mul(g[1], v2)), g[2]), w);
    float b = jf_mul(jf_add(jf_add(jf_mul(g[3], u2), jf_mul(g[4], v2)), g[5]), w);
    float ex = jf_sub(u1, a), ey = jf_sub(v1, b);
    const float chi1 = jf_mul(jf_add(jf_mul(ex, ex), jf_mul(ey, ey)), invS2);
    w = jd_f(jd_div(1.0, (double)jf_add(jf_add(jf_mul(h[6], u1), jf_mul(h[7], v1)), h[8])));
    a = jf_mul(jf_add(jf_add(jf_mul(h[0], u1), jf_mul(h[1], v1)), h[2]), w);
    b = jf_mul(jf_add(jf_add(jf_mul(h[3], u1), jf_mul(h[4], v1)), h[5]), w);
    ex = jf_sub(u2, a); ey = jf_sub(v2, b);
    const float chi2 = jf_mul(jf_add(jf_mul(ex, ex), jf_mul(ey, ey)), invS2);
    const bool o1 = chi1 > IN_TH, o2 = chi2 > IN_TH;
    t1 = o1 ? 0.f : jf_sub(IN_TH, chi1);
    t2 = o2 ? 0.f : jf_sub(IN_TH, chi2);
    in = !o1 && !o2;
}
// ... under CheckFundamental (:413-465)
IN_HD void in_check_f(const float* f, float u1, float v1, float u2, float v2, float invS2, float& t1, float& t2, bool& in)
{
    const float a2 = jf_add(jf_add(jf_mul(f[0], u1), jf_mul(f[1], v1)), f[2]);
    const float b2 = jf_add(jf_add(jf_mul(f[3], u1), jf_mul(f[4], v1)), f[5]);
    const float c2 = jf_add(jf_add(jf_mul(f[6], u1), jf_mul(f[7], v1)), f[8]);
    const float num2 = jf_add(jf_add(jf_mul(a2, u2), jf_mul(b2, v2)), c2);
    const float chi1 = jf_mul(jf_div(jf_mul(num2, num2), jf_add(jf_mul(a2, a2), jf_mul(b2, b2))), invS2);
    const float a1 = jf_add(jf_add(jf_mul(f[0], u2), jf_mul(f[3], v2)), f[6]);
    const float b1 = jf_add(jf_add(jf_mul(f[1], u2), jf_mul(f[4], v2)), f[7]);
    const float c1 = jf_add(jf_add(jf_mul(f[2], u2), jf_mul(f[5], v2)), f[8]);
    const float num1 = jf_add(jf_add(jf_mul(a1, u1), jf_mul(b1, v1)), c1);
    const float chi2 = jf_mul(jf_div(jf_mul(num1, num1), jf_add(jf_mul(a1, a1), jf_mul(b1, b1))), invS2);
    const bool o1 = chi1 > IN_TH_F, o2 = chi2 > IN_TH_F;
    t1 = o1 ? 0.f : jf_sub(IN_TH, chi1);
    t2 = o2 ? 0.f : jf_sub(IN_TH, chi2);
    in = !o1 && !o2;
}
IN_HD float in_inv_sigma2(float sigma) { return jd_f(jd_div(1.0, (double)jf_mul(sigma, sigma))); }

// ---- the reconstruction ----
struct InMotion { float R[9], t[3], P2[12], O2[3]; };
struct InCam { float fx, fy, cx, cy; };

// what CheckRT derives from (R, t) before its loop: P2 = K*[R | t] (the small path), O2 = -R.t()*t (as Frame::SetPose's mOw)
IN_HD void in_motion_finish(InMotion* m, const InCam& C)
{
    const float K[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) m->P2[4 * i + j] = in_small(in_dot3(K[3 * i], K[3 * i + 1], K[3 * i + 2], m->R[j], m->R[3 + j], m->R[6 + j]));
        m->P2[4 * i + 3] = in_small(in_dot3(K[3 * i], K[3 * i + 1], K[3 * i + 2], m->t[0], m->t[1], m->t[2]));
        m->O2[i] = jd_f(jd_mul((double)in_dot3(m->R[i], m->R[3 + i], m->R[6 + i], m->t[0], m->t[1], m->t[2]), -1.0));
    }
}

// ReconstructF's four hypotheses (:479-497, DecomposeE :909-929)
IN_HD void in_motions_f(const float* F21, const InCam& C, float* wsA, float* wsV, double* wsW, InMotion* M)
{
    const float K[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
    float X[9], E[9], w[3], U[9], Vt[9], R1[9], R2[9];
    in_mul33_t(K, F21, true, X);
    in_mul33(X, K, E);
    in_svd33<1>(E, wsA, wsV, wsW, w, U, Vt);
    float t[3] = {U[2], U[5], U[8]};
    in_scale3(t, jd_div(1.0, in_normd(t)));
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    in_mul33(U, W, X);
    in_mul33(X, Vt, R1);
    if (in_det33(R1) < 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    }
    in_mul33_t(U, W, false, X);
    in_mul33(X, Vt, R2);
    if (in_det33(R2) < 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    }
#pragma unroll
    for (int h = 0; h < 4; h++) {
#pragma unroll
        for (int i = 0; i < 9; i++) M[h].R[i] = (h & 1) ? R2[i] : R1[i];
#pragma unroll
        for (int i = 0; i < 3; i++) M[h].t[i] = h >= 2 ? -t[i] : t[i];
        in_motion_finish(M + h, C);
    }
}

// ReconstructH's eight hypotheses (:584-686); false = the d1/d2, d2/d3 test of :597
IN_HD bool in_motions_h(const float* H21, const InCam& C, float* wsA, float* wsV, double* wsW, InMotion* M)
{
    const float K[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
    float Ki[9], X[9], A[9], w[3], U[9], Vt[9];
    in_inv33(K, Ki);
    in_mul33(Ki, H21, X);
    in_mul33(X, K, A);
    in_svd33<1>(A, wsA, wsV, wsW, w, U, Vt);
    const float s = jd_f(jd_mul(in_det33(U), in_det33(Vt)));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)jf_div(d1, d2) < 1.00001 || (double)jf_div(d2, d3) < 1.00001) return false;
    const float q1 = jf_mul(d1, d1), q2 = jf_mul(d2, d2), q3 = jf_mul(d3, d3);
    const float aux1 = jf_sqrt(jf_div(jf_sub(q1, q2), jf_sub(q1, q3)));
    const float aux3 = jf_sqrt(jf_div(jf_sub(q2, q3), jf_sub(q1, q3)));
    const float root = jf_sqrt(jf_mul(jf_sub(q1, q2), jf_sub(q2, q3)));
    const float auxSt = jf_div(root, jf_mul(jf_add(d1, d3), d2));
    const float ct = jf_div(jf_add(q2, jf_mul(d1, d3)), jf_mul(jf_add(d1, d3), d2));
    const float auxSp = jf_div(root, jf_mul(jf_sub(d1, d3), d2));
    const float cp = jf_div(jf_sub(jf_mul(d1, d3), q2), jf_mul(jf_sub(d1, d3), d2));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int q = i & 3;
        const float x1 = q < 2 ? aux1 : -aux1, x3 = (q & 1) ? -aux3 : aux3;
        const float sg = (q == 0 || q == 3) ? 1.f : -1.f;               // stheta / sphi: {+, -, -, +}
        float Rp[9], tp[3], R[9];
        if (i < 4) {
            const float st = sg > 0 ? auxSt : -auxSt;
            const float r[9] = {ct, 0.f, -st, 0.f, 1.f, 0.f, st, 0.f, ct};
#pragma unroll
            for (int k = 0; k < 9; k++) Rp[k] = r[k];
            tp[0] = x1; tp[1] = 0.f; tp[2] = -x3;
            in_scale3(tp, (double)jf_sub(d1, d3));
        } else {
            const float sp = sg > 0 ? auxSp : -auxSp;
            const float r[9] = {cp, 0.f, sp, 0.f, -1.f, 0.f, sp, 0.f, -cp};
#pragma unroll
            for (int k = 0; k < 9; k++) Rp[k] = r[k];
            tp[0] = x1; tp[1] = 0.f; tp[2] = x3;
            in_scale3(tp, (double)jf_add(d1, d3));
        }
        in_mul33_alpha(U, Rp, s, X);
        in_mul33(X, Vt, R);
        float t[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = in_small(in_dot3(U[3 * k], U[3 * k + 1], U[3 * k + 2], tp[0], tp[1], tp[2]));
        in_scale3(t, jd_div(1.0, in_normd(t)));
#pragma unroll
        for (int k = 0; k < 9; k++) M[i].R[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) M[i].t[k] = t[k];
        in_motion_finish(M + i, C);
    }
    return true;
}

// One match under CheckRT (:830-894) with Triangulate (:734-747): bit 0 = counted in nGood (P3D written, the cosine pushed),
// bit 1 = vbGood.  wsA, wsV [16*S], wsW [4*S]: the 4 x 4 Jacobi's workspace.
template <int S>
IN_HD int in_check_rt(const InMotion* m, const InCam& C, float u1, float v1, float u2, float v2, float th2, float* wsA, float* wsV, double* wsW,
                      float* X, float& cosp)
{
    const float P1[12] = {C.fx, 0.f, C.cx, 0.f, 0.f, C.fy, C.cy, 0.f, 0.f, 0.f, 1.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        wsA[(4 * c + 0) * S] = jd_f(jd_add(jd_add(jd_mul((double)P1[8 + c], (double)u1), -(double)P1[c]), 0.0));
        wsA[(4 * c + 1) * S] = jd_f(jd_add(jd_add(jd_mul((double)P1[8 + c], (double)v1), -(double)P1[4 + c]), 0.0));
        wsA[(4 * c + 2) * S] = jd_f(jd_add(jd_add(jd_mul((double)m->P2[8 + c], (double)u2), -(double)m->P2[c]), 0.0));
        wsA[(4 * c + 3) * S] = jd_f(jd_add(jd_add(jd_mul((double)m->P2[8 + c], (double)v2), -(double)m->P2[4 + c]), 0.0));
    }
    jf_jacobi<4, 4, S>(wsA, wsV, wsW);
    X[0] = wsV[12 * S]; X[1] = wsV[13 * S]; X[2] = wsV[14 * S];
    in_scale3(X, jd_div(1.0, (double)wsV[15 * S]));
    cosp = 0.f;
    if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) return 0;
    const float n1[3] = {jf_sub(X[0], 0.f), jf_sub(X[1], 0.f), jf_sub(X[2], 0.f)};
    const float n2[3] = {jf_sub(X[0], m->O2[0]), jf_sub(X[1], m->O2[1]), jf_sub(X[2], m->O2[2])};
    const float dist1 = jd_f(in_normd(n1)), dist2 = jd_f(in_normd(n2));
    cosp = jd_f(jd_div(in_dotd(n1, n2), (double)jf_mul(dist1, dist2)));
    const bool far = !((double)cosp < 0.99998);
    if (X[2] <= 0 && !far) return 0;
    float X2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) X2[i] = in_small_c(in_dot3(m->R[3 * i], m->R[3 * i + 1], m->R[3 * i + 2], X[0], X[1], X[2]), m->t[i]);
    if (X2[2] <= 0 && !far) return 0;
    float iz = jd_f(jd_div(1.0, (double)X[2]));
    float ex = jf_sub(jf_add(jf_mul(jf_mul(C.fx, X[0]), iz), C.cx), u1), ey = jf_sub(jf_add(jf_mul(jf_mul(C.fy, X[1]), iz), C.cy), v1);
    if (jf_add(jf_mul(ex, ex), jf_mul(ey, ey)) > th2) return 0;
    iz = jd_f(jd_div(1.0, (double)X2[2]));
    ex = jf_sub(jf_add(jf_mul(jf_mul(C.fx, X2[0]), iz), C.cx), u2); ey = jf_sub(jf_add(jf_mul(jf_mul(C.fy, X2[1]), iz), C.cy), v2);
    if (jf_add(jf_mul(ex, ex), jf_mul(ey, ey)) > th2) return 0;
    return far ? 1 : 3;
}
IN_HD float in_th2(float sigma) { return jd_f(jd_mul(4.0, (double)jf_mul(sigma, sigma))); }
// acos(c)*180/CV_PI: the double acos of the float (the one operation the device need not reproduce bit for bit)
IN_HD float in_parallax(float c) { return jd_f(jd_div(jd_mul(acos((double)c), 180.0), 3.1415926535897932384626433832795)); }
// a float as an unsigned key of the same order, and back
IN_HD uint32_t in_key(float c) { const uint32_t u = __builtin_bit_cast(uint32_t, c); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
IN_HD float in_unkey(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// ReconstructF's decision (:499-569) over nGood[4], parallax[4]: the status bits and the hypothesis examined
IN_HD int in_decide_f(const int* nGood, const float* par, int N, float minParallax, int minTri, int& chosen)
{
    const int maxGood = max(nGood[0], max(nGood[1], max(nGood[2], nGood[3])));
    const int nMinGood = max((int)(0.9 * (double)N), minTri);
    int nsimilar = 0;
    chosen = -1;
#pragma unroll
    for (int i = 3; i >= 0; i--) { if ((double)nGood[i] > 0.7 * (double)maxGood) nsimilar++; if (nGood[i] == maxGood) chosen = i; }
    int status = 0;
    if (maxGood < nMinGood) status |= PGORB_INIT_FEW_GOOD;
    if (nsimilar > 1) status |= PGORB_INIT_AMBIGUOUS;
    if (!status) {
        float p = par[0];
#pragma unroll
        for (int i = 1; i < 4; i++) if (chosen == i) p = par[i];
        status = p > minParallax ? PGORB_INIT_OK : PGORB_INIT_LOW_PARALLAX;
    }
    return status;
}
// ReconstructH's (:689-731): every clause of :721 that fails sets its bit
IN_HD int in_decide_h(const int* nGood, const float* par, int N, float minParallax, int minTri, int& chosen)
{
    int best = 0, second = 0;
    float bestPar = -1.f;
    chosen = -1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (nGood[i] > best) { second = best; best = nGood[i]; chosen = i; bestPar = par[i]; }
        else if (nGood[i] > second) second = nGood[i];
    }
    int status = 0;
    if (!((double)second < 0.75 * (double)best)) status |= PGORB_INIT_AMBIGUOUS;
    if (!(bestPar >= minParallax)) status |= PGORB_INIT_LOW_PARALLAX;
    if (!(best > minTri) || !((double)best > 0.9 * (double)N)) status |= PGORB_INIT_FEW_GOOD;
    return status ? status : PGORB_INIT_OK;
}

// a complete pgorb_kf_pose from [R | t]: Frame::SetPose's mOw = -Rcw.t()*tcw, the camera copied (as pnp_put_pose)
IN_HD void in_put_pose(pgorb_kf_pose* o, const pgorb_kf_pose& cam, const float* R, const float* t)
{
    pgorb_kf_pose q = cam;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) q.Tcw[4 * r + c] = R[3 * r + c];
        q.Tcw[4 * r + 3] = t[r];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) q.Ow[i] = jd_f(jd_mul((double)in_dot3(R[i], R[3 + i], R[6 + i], t[0], t[1], t[2]), -1.0));
    *o = q;
}

// Normalize's T (:790-794) and the two matrices made of T2 (:134, :185)
IN_HD void in_make_T(float mx, float my, float sX, float sY, float* T)
{
    T[0] = sX; T[1] = 0.f; T[2] = jf_mul(-mx, sX); T[3] = 0.f; T[4] = sY; T[5] = jf_mul(-my, sY); T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ---- the kernels ----
struct InitBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap; const int32_t* pairF1; const int32_t* pairF2; const pgorb_kf_pose* cam;
    const int32_t* matches; const uint32_t* draws;
    float sigma, minParallax; int iters, minTri, words;
    // the scratch arena
    int32_t* nKept; int2* idx; float4* xy; float4* pn; float* T; pgorb_init_hypothesis* hyps; uint64_t* mask; float4* rt; uint8_t* rtFlag;
    // outputs
    pgorb_kf_pose* poseOut; float* P3D; uint8_t* tri; int32_t* matchesOut;
    pgorb_map_point* points; int32_t* kfPoint1; int32_t* kfPoint2; int32_t* obsStart; int32_t* obsFrame; int32_t* obsIdx; int32_t* npoints;
    pgorb_init_hypothesis* trace; int32_t* info; float* finfo;
};

// exclusive prefix of `flag` over the workgroup in thread order, and the total
__device__ __forceinline__ void init_block_prefix(bool flag, int* cnt, int& before, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    before = 0; total = 0;
#pragma unroll
    for (int w = 0; w < INIT_WAVES; w++) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
    __syncthreads();
    before += __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(INIT_T) void k_init_prepare(InitBatch B)
{
    __shared__ float sx[INIT_CHUNK], sy[INIT_CHUNK];
    __shared__ float sN[2][4];                                          // meanX, meanY, sX, sY of frame 1, frame 2
    __shared__ int cnt[INIT_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, cap = B.cap;
    const int f1 = B.pairF1[p], f2 = B.pairF2[p];
    const int n1 = min(max(B.n[f1], 0), cap), n2 = min(max(B.n[f2], 0), cap);
    for (int fr = 0; fr < 2; fr++) {
        const pgorb_keypoint* K = B.K + (int64_t)(fr ? f2 : f1) * cap;
        const int nf = fr ? n2 : n1;
        const float fn = (float)nf;
        float ax = 0.f, ay = 0.f;                                       // thread 0's ordered sums
        for (int c0 = 0; c0 < nf; c0 += INIT_CHUNK) {
            const int m = min(INIT_CHUNK, nf - c0);
            for (int i = tid; i < m; i += INIT_T) { sx[i] = K[c0 + i].x; sy[i] = K[c0 + i].y; }
            __syncthreads();
            if (tid == 0) for (int i = 0; i < m; i++) { ax = __fadd_rn(ax, sx[i]); ay = __fadd_rn(ay, sy[i]); }
            __syncthreads();
        }
        if (tid == 0) { sN[fr][0] = __fdiv_rn(ax, fn); sN[fr][1] = __fdiv_rn(ay, fn); }
        __syncthreads();
        const float mx = sN[fr][0], my = sN[fr][1];
        ax = 0.f; ay = 0.f;
        for (int c0 = 0; c0 < nf; c0 += INIT_CHUNK) {
            const int m = min(INIT_CHUNK, nf - c0);
            for (int i = tid; i < m; i += INIT_T) { sx[i] = fabsf(__fsub_rn(K[c0 + i].x, mx)); sy[i] = fabsf(__fsub_rn(K[c0 + i].y, my)); }
            __syncthreads();
            if (tid == 0) for (int i = 0; i < m; i++) { ax = __fadd_rn(ax, sx[i]); ay = __fadd_rn(ay, sy[i]); }
            __syncthreads();
        }
        if (tid == 0) {
            sN[fr][2] = jd_f(jd_div(1.0, (double)__fdiv_rn(ax, fn)));
            sN[fr][3] = jd_f(jd_div(1.0, (double)__fdiv_rn(ay, fn)));
        }
        __syncthreads();
    }
    if (tid == 0) {
        float T1[9], T2[9], T2inv[9];
        in_make_T(sN[0][0], sN[0][1], sN[0][2], sN[0][3], T1);
        in_make_T(sN[1][0], sN[1][1], sN[1][2], sN[1][3], T2);
        in_inv33(T2, T2inv);
        float* T = B.T + (int64_t)p * 27;
#pragma unroll
        for (int i = 0; i < 9; i++) { T[i] = T1[i]; T[9 + i] = T2inv[i]; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) T[18 + 3 * r + c] = T2[3 * c + r];
    }
    const int64_t row = (int64_t)p * cap;
    const pgorb_keypoint* K1 = B.K + (int64_t)f1 * cap;
    const pgorb_keypoint* K2 = B.K + (int64_t)f2 * cap;
    int N = 0;
    for (int i0 = 0; i0 < cap; i0 += INIT_T) {
        const int i = i0 + tid;
        int m = i < n1 ? B.matches[row + i] : -1;
        if (m < 0 || m >= n2) m = -1;                                   // (a bad index counts as no match)
        int before, total;
        init_block_prefix(m >= 0, cnt, before, total);
        if (m >= 0) {
            const int64_t k = row + N + before;
            const float u1 = K1[i].x, v1 = K1[i].y, u2 = K2[m].x, v2 = K2[m].y;
            B.idx[k] = make_int2(i, m);
            B.xy[k] = make_float4(u1, v1, u2, v2);
            B.pn[k] = make_float4(__fmul_rn(__fsub_rn(u1, sN[0][0]), sN[0][2]), __fmul_rn(__fsub_rn(v1, sN[0][1]), sN[0][3]),
                                  __fmul_rn(__fsub_rn(u2, sN[1][0]), sN[1][2]), __fmul_rn(__fsub_rn(v2, sN[1][1]), sN[1][3]));
        }
        N += total;
    }
    if (tid == 0) B.nKept[p] = N;
}

__global__ __launch_bounds__(64) void k_init_hypotheses(InitBatch B)
{
    __shared__ float sA[9 * 16];                                        // H: At (9 rows of 16); F: A and its completion row (9 rows of 9)
    __shared__ float sV[81];                                            // H: Vt; F: the 3 x 3 workspace
    __shared__ double sW[9];
    __shared__ float sM[18];                                            // H21i, H12i or F21i for the scoring lanes
    const int it = blockIdx.x, model = blockIdx.y, p = blockIdx.z, lane = threadIdx.x;
    const int N = B.nKept[p];
    const int64_t row = (int64_t)p * B.cap;
    pgorb_init_hypothesis* H = B.hyps + (int64_t)p * B.iters + it;
    pgorb_init_hypothesis* Tr = B.trace ? B.trace + (int64_t)p * B.iters + it : nullptr;
    uint64_t* mask = B.mask + (((int64_t)p * B.iters + it) * 2 + model) * B.words;
    float* Mo = model ? H->F21 : H->H21;
    float* Mt = Tr ? (model ? Tr->F21 : Tr->H21) : nullptr;
    if (N < 8) {                                                         // FEW: nothing is evaluated
        if (lane < 9) { Mo[lane] = 0.f; if (Mt) Mt[lane] = 0.f; }
        if (lane == 0) {
            if (model) { H->scoreF = 0.f; H->inliersF = 0; if (Tr) { Tr->scoreF = 0.f; Tr->inliersF = 0; } }
            else { H->scoreH = 0.f; H->inliersH = 0; if (Tr) { Tr->scoreH = 0.f; Tr->inliersH = 0; } }
        }
        if (!model && lane < 8) { H->set[lane] = 0; if (Tr) Tr->set[lane] = 0; }
        return;
    }
    const float4* pn = B.pn + row;
    const float* T = B.T + (int64_t)p * 27;
    if (lane == 0) {
        int sel[8];
        in_select8(B.draws + ((int64_t)p * B.iters + it) * 8, N, sel);
        float T1[9], T2x[9], M[9], Mi[9];
#pragma unroll
        for (int i = 0; i < 9; i++) { T1[i] = T[i]; T2x[i] = T[(model ? 18 : 9) + i]; }
        if (!model) {
#pragma unroll
            for (int j = 0; j < 8; j++) { const float4 q = pn[sel[j]]; in_h_rows(sA, j, q.x, q.y, q.z, q.w); H->set[j] = sel[j]; if (Tr) Tr->set[j] = sel[j]; }
            in_solve_h(sA, sV, sW, T1, T2x, M, Mi);
#pragma unroll
            for (int i = 0; i < 9; i++) { sM[i] = M[i]; sM[9 + i] = Mi[i]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) { const float4 q = pn[sel[j]]; in_f_row(sA, j, q.x, q.y, q.z, q.w); }
            in_solve_f(sA, sV, sV + 9, sW, T1, T2x, M);
#pragma unroll
            for (int i = 0; i < 9; i++) sM[i] = M[i];
        }
    }
    __syncthreads();
    float M[9], Mi[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = sM[i]; Mi[i] = model ? 0.f : sM[9 + i]; }
    const float invS2 = in_inv_sigma2(B.sigma);
    const float4* xy = B.xy + row;
    float score = 0.f;
    int inl = 0;
    for (int e0 = 0; e0 < N; e0 += 64) {
        const int e = e0 + lane;
        float t1 = 0.f, t2 = 0.f;
        bool in = false;
        if (e < N) {
            const float4 q = xy[e];
            if (model) in_check_f(M, q.x, q.y, q.z, q.w, invS2, t1, t2, in);
            else in_check_h(M, Mi, q.x, q.y, q.z, q.w, invS2, t1, t2, in);
        }
        const unsigned long long bal = __ballot(in);
        inl += __popcll(bal);
        if (lane == 0) mask[e0 >> 6] = bal;
        // the reference's ONE sequential sum: term 1 then term 2 of each match in index order (a skipped term adds +0, exactly)
        const int i1 = __float_as_int(t1), i2 = __float_as_int(t2);
#pragma unroll
        for (int l = 0; l < 64; l++) {
            score = __fadd_rn(score, __int_as_float(__builtin_amdgcn_readlane(i1, l)));
            score = __fadd_rn(score, __int_as_float(__builtin_amdgcn_readlane(i2, l)));
        }
    }
    if (lane < 9) { Mo[lane] = M[lane]; if (Mt) Mt[lane] = M[lane]; }
    if (lane == 0) {
        if (model) { H->scoreF = score; H->inliersF = inl; if (Tr) { Tr->scoreF = score; Tr->inliersF = inl; } }
        else { H->scoreH = score; H->inliersH = inl; if (Tr) { Tr->scoreH = score; Tr->inliersH = inl; } }
    }
}

__global__ __launch_bounds__(INIT_T) void k_init_reconstruct(InitBatch B)
{
    __shared__ float wsA[16 * INIT_T], wsV[16 * INIT_T];               // one 4 x 4 Jacobi per thread, element-major
    __shared__ double wsW[4 * INIT_T];
    __shared__ float s3A[9], s3V[9];                                    // thread 0's 3 x 3 decompositions
    __shared__ double s3W[3];
    __shared__ InMotion mot[8];
    __shared__ int cnt[INIT_WAVES];
    __shared__ int sI[8];                                               // status, nh, best H, best F, chosen, model's best iteration
    __shared__ int sGood[8];
    __shared__ float sPar[8], sF[3];
    const int p = blockIdx.x, tid = threadIdx.x, cap = B.cap;
    const int N = B.nKept[p];
    const int64_t row = (int64_t)p * cap;
    const int f1 = B.pairF1[p], f2 = B.pairF2[p];
    const pgorb_kf_pose camPose = B.cam[f1];
    const InCam C = {camPose.fx, camPose.fy, camPose.cx, camPose.cy};
    const pgorb_init_hypothesis* H = B.hyps + (int64_t)p * B.iters;
    if (tid < 8) { sGood[tid] = 0; sPar[tid] = 0.f; }
    if (tid == 0) {
        int status = 0, nh = 0, bH = -1, bF = -1;
        float SH = 0.f, SF = 0.f, RH = 0.f;
        if (N < 8) status = PGORB_INIT_FEW;
        else {
            for (int k = 0; k < B.iters; k++) {                         // the first strict maximum above 0 (a NaN compares false)
                if (H[k].scoreH > SH) { SH = H[k].scoreH; bH = k; }
                if (H[k].scoreF > SF) { SF = H[k].scoreF; bF = k; }
            }
            if (SH == 0.f && SF == 0.f) status = PGORB_INIT_NO_MODEL;
            else {
                RH = __fdiv_rn(SH, __fadd_rn(SH, SF));
                if ((double)RH > 0.40) {
                    status = PGORB_INIT_MODEL_H;
                    float M[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) M[i] = H[bH].H21[i];
                    if (in_motions_h(M, C, s3A, s3V, s3W, mot)) nh = 8;
                    else status |= PGORB_INIT_DEGENERATE_H;
                } else {
                    status = PGORB_INIT_MODEL_F;
                    float M[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) M[i] = H[bF].F21[i];
                    in_motions_f(M, C, s3A, s3V, s3W, mot);
                    nh = 4;
                }
            }
        }
        sI[0] = status; sI[1] = nh; sI[2] = bH; sI[3] = bF; sI[4] = -1;
        sI[5] = (status & PGORB_INIT_MODEL_H) ? bH : ((status & PGORB_INIT_MODEL_F) ? bF : -1);
        sF[0] = SH; sF[1] = SF; sF[2] = RH;
    }
    __syncthreads();
    const int nh = sI[1], bIt = sI[5];
    const int model = (sI[0] & PGORB_INIT_MODEL_F) ? 1 : 0;
    const uint64_t* mask = bIt >= 0 ? B.mask + (((int64_t)p * B.iters + bIt) * 2 + model) * B.words : nullptr;
    const float4* xy = B.xy + row;
    float4* rt = B.rt + row * 8;
    uint8_t* rtF = B.rtFlag + row * 8;
    // CheckRT: the threads over (hypothesis, match)
    const float th2 = in_th2(B.sigma);
    for (int e0 = 0; e0 < nh * N; e0 += INIT_T) {
        const int e = e0 + tid;
        if (e < nh * N) {
            const int h = e / N, k = e - h * N;
            int fl = 0;
            float X[3] = {0.f, 0.f, 0.f}, cosp = 0.f;
            if ((mask[k >> 6] >> (k & 63)) & 1ull) {
                const float4 q = xy[k];
                fl = in_check_rt<INIT_T>(mot + h, C, q.x, q.y, q.z, q.w, th2, wsA + tid, wsV + tid, wsW + tid, X, cosp);
            }
            rt[(int64_t)h * cap + k] = make_float4(X[0], X[1], X[2], cosp);
            rtF[(int64_t)h * cap + k] = (uint8_t)fl;
        }
    }
    __syncthreads();
    // the chosen model's inlier count; per hypothesis nGood and the order statistic of the cosines
    int Nm = 0;
    if (mask) for (int k0 = 0; k0 < N; k0 += INIT_T) { const int k = k0 + tid; Nm += __syncthreads_count(k < N && ((mask[k >> 6] >> (k & 63)) & 1ull)); }
    for (int h = 0; h < nh; h++) {
        const float4* rh = rt + (int64_t)h * cap;
        const uint8_t* fh = rtF + (int64_t)h * cap;
        int nGood = 0;
        for (int k0 = 0; k0 < N; k0 += INIT_T) { const int k = k0 + tid; nGood += __syncthreads_count(k < N && (fh[k] & 1)); }
        float par = 0.f;
        if (nGood > 0) {
            const int want = min(50, nGood - 1);
            uint32_t prefix = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t cand = prefix | (1u << bit);
                int below = 0;
                for (int k0 = 0; k0 < N; k0 += INIT_T) { const int k = k0 + tid; below += __syncthreads_count(k < N && (fh[k] & 1) && in_key(rh[k].w) < cand); }
                if (below <= want) prefix = cand;
            }
            par = in_parallax(in_unkey(prefix));
        }
        if (tid == 0) { sGood[h] = nGood; sPar[h] = par; }
    }
    __syncthreads();
    if (tid == 0) {
        int status = sI[0], chosen = -1;
        if (nh == 8) status |= in_decide_h(sGood, sPar, Nm, B.minParallax, B.minTri, chosen);
        else if (nh == 4) status |= in_decide_f(sGood, sPar, Nm, B.minParallax, B.minTri, chosen);
        sI[0] = status; sI[4] = chosen;
        int32_t* I = B.info + (int64_t)p * PGORB_INIT_INFO;
        I[0] = status; I[1] = N; I[2] = sI[2]; I[3] = sI[2] >= 0 ? H[sI[2]].inliersH : 0; I[4] = sI[3]; I[5] = sI[3] >= 0 ? H[sI[3]].inliersF : 0;
        I[6] = chosen;
        for (int i = 0; i < 8; i++) I[7 + i] = sGood[i];
        I[15] = Nm;
        float* Fi = B.finfo + (int64_t)p * PGORB_INIT_FINFO;
        Fi[0] = sF[0]; Fi[1] = sF[1]; Fi[2] = sF[2];
        for (int i = 0; i < 8; i++) Fi[3 + i] = sPar[i];
        pgorb_kf_pose* po = B.poseOut + (int64_t)p * 2;
        if (status & PGORB_INIT_OK) {
            const float I3[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, z3[3] = {0.f, 0.f, 0.f};
            in_put_pose(po, camPose, I3, z3);
            in_put_pose(po + 1, camPose, mot[chosen].R, mot[chosen].t);
        } else {
            pgorb_kf_pose z; memset(&z, 0, sizeof(z)); po[0] = z; po[1] = z;
        }
    }
    __syncthreads();
    const bool ok = (sI[0] & PGORB_INIT_OK) != 0;
    const int chosen = sI[4];
    // every per-keypoint output cleared, then written by match
    for (int i = tid; i < cap; i += INIT_T) {
        B.P3D[(row + i) * 3] = 0.f; B.P3D[(row + i) * 3 + 1] = 0.f; B.P3D[(row + i) * 3 + 2] = 0.f;
        B.tri[row + i] = 0; B.matchesOut[row + i] = -1;
        if (B.points) {
            pgorb_map_point z; memset(&z, 0, sizeof(z));
            B.points[row + i] = z; B.kfPoint1[row + i] = -1; B.kfPoint2[row + i] = -1;
            B.obsFrame[2 * (row + i)] = -1; B.obsFrame[2 * (row + i) + 1] = -1; B.obsIdx[2 * (row + i)] = -1; B.obsIdx[2 * (row + i) + 1] = -1;
        }
    }
    __syncthreads();
    int np = 0;
    if (ok) {
        const float4* rh = rt + (int64_t)chosen * cap;
        const uint8_t* fh = rtF + (int64_t)chosen * cap;
        const int2* idx = B.idx + row;
        for (int k0 = 0; k0 < N; k0 += INIT_T) {
            const int k = k0 + tid;
            const int fl = k < N ? fh[k] : 0;
            int before, total;
            init_block_prefix((fl & 2) != 0, cnt, before, total);
            if (fl & 1) {
                const int2 m = idx[k];
                const float4 X = rh[k];
                B.P3D[(row + m.x) * 3] = X.x; B.P3D[(row + m.x) * 3 + 1] = X.y; B.P3D[(row + m.x) * 3 + 2] = X.z;
                if (fl & 2) {
                    B.tri[row + m.x] = 1; B.matchesOut[row + m.x] = m.y;
                    if (B.points) {
                        const int s = np + before;
                        pgorb_map_point q; memset(&q, 0, sizeof(q));
                        q.pos[0] = X.x; q.pos[1] = X.y; q.pos[2] = X.z;
                        B.points[row + s] = q; B.kfPoint1[row + m.x] = s;
                        B.obsFrame[2 * (row + s)] = f1; B.obsFrame[2 * (row + s) + 1] = f2;
                        B.obsIdx[2 * (row + s)] = m.x; B.obsIdx[2 * (row + s) + 1] = m.y;
                    }
                }
            }
            np += total;
        }
        // frame 2's slots, by one lane in CreateInitialMapMonocular's loop order: a keypoint matched twice keeps the later point
        if (B.points && tid == 0) {
            int s = 0;
            for (int k = 0; k < N; k++)
                if (fh[k] & 2) B.kfPoint2[row + idx[k].y] = s++;
        }
    }
    if (B.points) for (int i = tid; i <= cap; i += INIT_T) B.obsStart[(int64_t)p * (cap + 1) + i] = 2 * min(i, np);
    if (tid == 0) { B.info[(int64_t)p * PGORB_INIT_INFO + 16] = np; if (B.npoints) B.npoints[p] = np; }
}

static const char* init_params_why(const pgorb_init_params* P)
{
    if (!P) return "params is NULL";
    if (!(P->sigma > 0.0f) || !std::isfinite(P->sigma)) return "sigma is not positive and finite";
    if (P->max_iterations < 1) return "max_iterations is below 1";
    if (!std::isfinite(P->min_parallax)) return "min_parallax is not finite";
    return nullptr;
}

extern "C" {

int pgorb_initializer_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap, const int32_t* d_pair_f1,
        const int32_t* d_pair_f2, int npairs, const pgorb_kf_pose* d_camera, const int32_t* d_matches12, const pgorb_init_params* params,
        const uint32_t* d_draws, pgorb_kf_pose* d_pose_out, float* d_P3D, uint8_t* d_triangulated, int32_t* d_matches12_out,
        pgorb_map_point* d_points, int32_t* d_kf_point1, int32_t* d_kf_point2, int32_t* d_obs_start, int32_t* d_obs_frame, int32_t* d_obs_idx,
        int32_t* d_npoints, pgorb_init_hypothesis* d_trace, int32_t* d_info, float* d_finfo, void* stream)
{
    if (!c) return PGORB_E_ARG;
    const bool anyMap = d_points || d_kf_point1 || d_kf_point2 || d_obs_start || d_obs_frame || d_obs_idx || d_npoints;
    const bool allMap = d_points && d_kf_point1 && d_kf_point2 && d_obs_start && d_obs_frame && d_obs_idx && d_npoints;
    if (!d_kps || !d_n || cap < 1 || npairs < 0 || anyMap != allMap ||
        (npairs && (!d_pair_f1 || !d_pair_f2 || !d_camera || !d_matches12 || !d_draws || !d_pose_out || !d_P3D || !d_triangulated ||
                    !d_matches12_out || !d_info || !d_finfo)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_initializer_batch_device");
    if (const char* why = init_params_why(params)) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_initializer: ") + why).c_str());
    if (cap > INIT_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_initializer: more than 16000 keypoints per frame");
    if (params->max_iterations > PGORB_INIT_MAX_ITERATIONS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_initializer: max_iterations above PGORB_INIT_MAX_ITERATIONS");
    if (!npairs) return 0;
    if (npairs > 65535) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_initializer: more than 65535 pairs");
    hipStream_t s = (hipStream_t)stream;
    InitBatch B;
    memset(&B, 0, sizeof(B));
    B.iters = params->max_iterations; B.words = (cap + 63) / 64;
    PgCarve L;
    const size_t np = (size_t)npairs;
    const size_t oN = L.take(np * 4), oIdx = L.take(np * cap * sizeof(int2)), oXy = L.take(np * cap * sizeof(float4)),
                 oPn = L.take(np * cap * sizeof(float4)), oT = L.take(np * 27 * 4), oHyp = L.take(np * B.iters * sizeof(pgorb_init_hypothesis)),
                 oMask = L.take(np * B.iters * 2 * B.words * 8), oRt = L.take(np * 8 * cap * sizeof(float4)), oRtF = L.take(np * 8 * cap);
    void* scr;
    int rc;
    if ((rc = pg_ctx_scratch(c, L.o, s, &scr))) return rc;
    uint8_t* base = (uint8_t*)scr;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.pairF1 = d_pair_f1; B.pairF2 = d_pair_f2; B.cam = d_camera; B.matches = d_matches12; B.draws = d_draws;
    B.sigma = params->sigma; B.minParallax = params->min_parallax; B.minTri = params->min_triangulated;
    B.nKept = (int32_t*)(base + oN); B.idx = (int2*)(base + oIdx); B.xy = (float4*)(base + oXy); B.pn = (float4*)(base + oPn);
    B.T = (float*)(base + oT); B.hyps = (pgorb_init_hypothesis*)(base + oHyp); B.mask = (uint64_t*)(base + oMask);
    B.rt = (float4*)(base + oRt); B.rtFlag = base + oRtF;
    B.poseOut = d_pose_out; B.P3D = d_P3D; B.tri = d_triangulated; B.matchesOut = d_matches12_out;
    B.points = d_points; B.kfPoint1 = d_kf_point1; B.kfPoint2 = d_kf_point2; B.obsStart = d_obs_start; B.obsFrame = d_obs_frame;
    B.obsIdx = d_obs_idx; B.npoints = d_npoints; B.trace = d_trace; B.info = d_info; B.finfo = d_finfo;
    hipLaunchKernelGGL(k_init_prepare, dim3((unsigned)npairs), dim3(INIT_T), 0, s, B);
    hipLaunchKernelGGL(k_init_hypotheses, dim3((unsigned)B.iters, 2u, (unsigned)npairs), dim3(64), 0, s, B);
    hipLaunchKernelGGL(k_init_reconstruct, dim3((unsigned)npairs), dim3(INIT_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "an Initializer kernel launch failed");
    return pg_ctx_scratch_done(c, s);
}

int pgorb_initializer(pgorb_ctx* c, const pgorb_keypoint* kps1, int n1, const pgorb_keypoint* kps2, int n2, const pgorb_kf_pose* camera,
        const int32_t* matches12, const pgorb_init_params* params, const uint32_t* draws, pgorb_kf_pose* pose_out, float* P3D,
        uint8_t* triangulated, int32_t* matches12_out, pgorb_map_point* points, int32_t* kf_point1, int32_t* kf_point2, int32_t* obs_start,
        int32_t* obs_frame, int32_t* obs_idx, int32_t* npoints, pgorb_init_hypothesis* trace, int32_t* info, float* finfo)
{
    if (!c) return PGORB_E_ARG;
    const bool anyMap = points || kf_point1 || kf_point2 || obs_start || obs_frame || obs_idx || npoints;
    const bool allMap = npoints && obs_start && (!n1 || (points && kf_point1 && obs_frame && obs_idx)) && (!n2 || kf_point2);
    const char* why = nullptr;
    if (n1 < 0 || n2 < 0) why = "a count is negative";
    else if (!camera || !params || !draws || !pose_out || !info || !finfo || (n1 && (!kps1 || !matches12 || !P3D || !triangulated || !matches12_out)) ||
             (n2 && !kps2) || (anyMap && !allMap))
        why = "an array that is read or written is NULL";
    else why = init_params_why(params);
    if (!why && !(std::isfinite(camera->fx) && std::isfinite(camera->fy) && std::isfinite(camera->cx) && std::isfinite(camera->cy)))
        why = "the camera is not finite";
    for (int i = 0; !why && i < n1; i++) {
        if (matches12[i] < -1 || matches12[i] >= n2) why = "matches12 is outside [-1, n2)";
        else if (!std::isfinite(kps1[i].x) || !std::isfinite(kps1[i].y)) why = "a keypoint coordinate is not finite";
    }
    for (int i = 0; !why && i < n2; i++)
        if (!std::isfinite(kps2[i].x) || !std::isfinite(kps2[i].y)) why = "a keypoint coordinate is not finite";
    const int iters = why ? 0 : params->max_iterations;
    if (!why && iters <= PGORB_INIT_MAX_ITERATIONS)
        for (int64_t k = 0; k < (int64_t)iters * 8; k++)
            if (draws[k] >= 0x80000000u) { why = "a draw is not below 2^31"; break; }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_initializer: ") + why).c_str());
    if (n1 > INIT_MAX_N || n2 > INIT_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_initializer: more than 16000 keypoints per frame");
    if (iters > PGORB_INIT_MAX_ITERATIONS) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_initializer: max_iterations above PGORB_INIT_MAX_ITERATIONS");
    const int cap = std::max(std::max(n1, n2), 1);
    const size_t kb = (size_t)cap * sizeof(pgorb_keypoint), nt = trace ? (size_t)iters * sizeof(pgorb_init_hypothesis) : 0;
    const size_t mp = anyMap ? 1 : 0;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 32), oK = s.region(PG_UP, 2 * kb), oCam = s.region(PG_UP, 2 * sizeof(pgorb_kf_pose)),
                 oM = s.region(PG_UP, (size_t)cap * 4), oD = s.region(PG_UP, (size_t)iters * 32),
                 oPose = s.region(PG_DOWN, 2 * sizeof(pgorb_kf_pose)), oP = s.region(PG_DOWN, (size_t)cap * 12), oTri = s.region(PG_DOWN, cap),
                 oMo = s.region(PG_DOWN, (size_t)cap * 4), oPts = s.region(PG_DOWN, mp * cap * sizeof(pgorb_map_point)),
                 oK1 = s.region(PG_DOWN, mp * cap * 4), oK2 = s.region(PG_DOWN, mp * cap * 4), oOs = s.region(PG_DOWN, mp * (cap + 1) * 4),
                 oOf = s.region(PG_DOWN, mp * cap * 8), oOi = s.region(PG_DOWN, mp * cap * 8), oNp = s.region(PG_DOWN, 64),
                 oT = s.region(PG_DOWN, nt), oI = s.region(PG_DOWN, PGORB_INIT_INFO * 4), oF = s.region(PG_DOWN, PGORB_INIT_FINFO * 4);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t hdr[8] = {n1, n2, 0, 1, 0, 0, 0, 0};                  // d_n [2], d_pair_f1 at +2, d_pair_f2 at +3
    s.put(oN, hdr, 32);
    s.put(oK, kps1, (size_t)n1 * sizeof(pgorb_keypoint), 0, kb);
    s.put(oK, kps2, (size_t)n2 * sizeof(pgorb_keypoint), kb, kb);
    s.put(oCam, camera, sizeof(pgorb_kf_pose));
    s.put(oCam, camera, sizeof(pgorb_kf_pose), sizeof(pgorb_kf_pose));
    memset(s.host(oM), 0xFF, (size_t)cap * 4);
    s.put(oM, matches12, (size_t)n1 * 4);
    s.put(oD, draws, (size_t)iters * 32);
    if ((rc = s.run([&] {
            return pgorb_initializer_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), cap, s.dev<int32_t>(oN) + 2, s.dev<int32_t>(oN) + 3, 1,
                s.dev<pgorb_kf_pose>(oCam), s.dev<int32_t>(oM), params, s.dev<uint32_t>(oD), s.dev<pgorb_kf_pose>(oPose), s.dev<float>(oP),
                s.dev(oTri), s.dev<int32_t>(oMo), mp ? s.dev<pgorb_map_point>(oPts) : nullptr, mp ? s.dev<int32_t>(oK1) : nullptr,
                mp ? s.dev<int32_t>(oK2) : nullptr, mp ? s.dev<int32_t>(oOs) : nullptr, mp ? s.dev<int32_t>(oOf) : nullptr,
                mp ? s.dev<int32_t>(oOi) : nullptr, mp ? s.dev<int32_t>(oNp) : nullptr, trace ? s.dev<pgorb_init_hypothesis>(oT) : nullptr,
                s.dev<int32_t>(oI), s.dev<float>(oF), nullptr); }))) return rc;
    memcpy(pose_out, s.host(oPose), 2 * sizeof(pgorb_kf_pose));
    if (n1) { memcpy(P3D, s.host(oP), (size_t)n1 * 12); memcpy(triangulated, s.host(oTri), n1); memcpy(matches12_out, s.host(oMo), (size_t)n1 * 4); }
    if (mp) {
        if (n1) {
            memcpy(points, s.host(oPts), (size_t)n1 * sizeof(pgorb_map_point)); memcpy(kf_point1, s.host(oK1), (size_t)n1 * 4);
            memcpy(obs_frame, s.host(oOf), (size_t)n1 * 8); memcpy(obs_idx, s.host(oOi), (size_t)n1 * 8);
        }
        if (n2) memcpy(kf_point2, s.host(oK2), (size_t)n2 * 4);
        memcpy(obs_start, s.host(oOs), (size_t)(n1 + 1) * 4);
        *npoints = *s.host<int32_t>(oNp);
    }
    if (trace) memcpy(trace, s.host(oT), nt);
    memcpy(info, s.host(oI), PGORB_INIT_INFO * 4);
    memcpy(finfo, s.host(oF), PGORB_INIT_FINFO * 4);
    return info[16];
}

}  // extern "C"
