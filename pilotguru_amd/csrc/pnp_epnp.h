// pnp_epnp.h -- the EPnP under PnPsolver::compute_pose (thirdparty/orb-slam2/src/PnPsolver.cc:375-950) as ONE definition that a
// group of threads runs together: a wave of the hypothesis kernel, a workgroup of the selection kernel's Refine, or a single
// host thread (lane 0 of 1: the same doubles, used to check the definition without a device).
//
// A 4-point hypothesis depends on the null-space basis the SVD happens to produce, so every double here
// is formed by a fixed operation on fixed operands, in the order tests/pnp_reference.py writes down: contraction is off
// (Makefile), fp64 + - * / sqrt are IEEE on both sides, and nothing here needs a transcendental.  Threads only share out
// INDEPENDENT elements (the entries of a matrix, the elements of two rotated rows, the correspondences); every sum runs from 0
// in index order inside one thread.  Control flow is uniform: every decision is taken from values all threads read alike, so a
// barrier stands between every phase that reads shared values and the writes that follow it.
//
// cvSVD / cvSolve(CV_SVD) / cvInvert(CV_SVD) are READ as OpenCV 2.4's JacobiSVDImpl_<double> (lapack.cpp), as mapping.hip's
// cnm_svd_v3 reads the float instance: one-sided Hestenes on the rows of A^T, cyclic (i, j), i < j; gamma without hypot.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNP_BAR() __syncthreads()
#define PNP_SQRT(x) __dsqrt_rn(x)
#else
#define PNP_BAR() ((void)0)
#define PNP_SQRT(x) sqrt(x)
#endif

#define PNP_DBL_EPSILON 2.220446049250313e-16
#define PNP_DBL_MIN 2.2250738585072014e-308
#define PNP_PT_DOUBLES 13                 // per correspondence: pws 3, us 2, alphas 4, pcs 3, one reprojection term

struct PnpCam { double fu, fv, uc, vc; };
// the per-correspondence arrays of one compute_pose (LDS for 4 points, the scratch arena for Refine)
struct PnpPts { double* pws; double* us; double* alphas; double* pcs; double* term; int n; };
PNP_HD PnpPts pnp_pts(double* base, int n, int cap)
{
    PnpPts P;
    P.pws = base; P.us = base + 3 * (long long)cap; P.alphas = base + 5 * (long long)cap; P.pcs = base + 9 * (long long)cap;
    P.term = base + 12 * (long long)cap; P.n = n;
    return P;
}
// the state the threads share (LDS on the device)
struct PnpWork {
    double At[144];                       // MtM, then Ut (rows 11..8 = the null-space vectors EPnP reads)
    double sA[30], sV[25], sW[12];        // the small decompositions: rows of A^T, Vt, W
    double cws[12], ccs[12], ci[9], L[60], rho[6], pc0[3], pw0[3];
    double R[3][9], t[3][3], err[3];      // the three candidates
    double Rb[9], tb[3];                  // the chosen one
};

// JacobiSVDImpl_<double>: At = n rows of length m (the rows of A^T), Vt n x n or null.  Leaves W descending, At's rows scaled
// to unit length (U^T; a row with W <= DBL_MIN is left as it is) and Vt's rows in the same order.
PNP_HD void pnp_svd(double* At, int m, int n, double* Vt, double* W, int lane, int nth)
{
    const double eps = PNP_DBL_EPSILON * 10;
    const int sweeps = m > 30 ? m : 30;          // a NaN matrix rotates for ever otherwise
    if (Vt) for (int k = lane; k < n * n; k += nth) Vt[k] = k / n == k % n ? 1.0 : 0.0;
    PNP_BAR();
    for (int it = 0; it < sweeps; it++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double* Ai = At + i * m;
                double* Aj = At + j * m;
                double a = 0.0, b = 0.0, p = 0.0;
                for (int k = 0; k < m; k++) { a += Ai[k] * Ai[k]; b += Aj[k] * Aj[k]; p += Ai[k] * Aj[k]; }
                if (fabs(p) <= eps * PNP_SQRT(a * b)) continue;
                p *= 2.0;
                const double beta = a - b, gamma = PNP_SQRT(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = PNP_SQRT(delta / gamma);
                    c = p / ((gamma * s) * 2.0);
                } else {
                    c = PNP_SQRT((gamma + beta) / (gamma * 2.0));
                    s = p / ((gamma * c) * 2.0);
                }
                PNP_BAR();                        // every thread has read both rows
                for (int k = lane; k < m + (Vt ? n : 0); k += nth) {
                    double* x = k < m ? Ai + k : Vt + i * n + (k - m);
                    double* y = k < m ? Aj + k : Vt + j * n + (k - m);
                    const double x0 = *x, y0 = *y;
                    *x = c * x0 + s * y0;
                    *y = (-s) * x0 + c * y0;
                }
                PNP_BAR();
                changed = true;
            }
        if (!changed) break;
    }
    PNP_BAR();                                    // the skipped pairs of the last sweep only read: every thread is through before the rows move
    if (lane == 0) {
        for (int i = 0; i < n; i++) {
            double sd = 0.0;
            for (int k = 0; k < m; k++) sd += At[i * m + k] * At[i * m + k];
            W[i] = PNP_SQRT(sd);
        }
        for (int i = 0; i < n - 1; i++) {
            int j = i;
            for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
            if (i != j) {
                double x = W[i]; W[i] = W[j]; W[j] = x;
                for (int k = 0; k < m; k++) { x = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = x; }
                if (Vt) for (int k = 0; k < n; k++) { x = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = x; }
            }
        }
        for (int i = 0; i < n; i++)
            if (W[i] > PNP_DBL_MIN) {
                const double s = 1.0 / W[i];
                for (int k = 0; k < m; k++) At[i * m + k] *= s;
            }
    }
    PNP_BAR();
}

PNP_HD double pnp_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PNP_HD double pnp_dist2(const double* a, const double* b)
{
    return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2]);
}

// qr_solve (:860-950) on a 6 x 4 A, in place; false (X as it was) where a column's eta is 0.  The reference's scan for eta reads
// before it steps, so it covers rows k .. nr-2.
PNP_HD bool pnp_qr_solve(double A[6][4], double* b, double* X)
{
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k][k]);
        for (int i = k; i < nr - 1; i++) { const double elt = fabs(A[i][k]); if (eta < elt) eta = elt; }
        if (eta == 0) return false;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < nr; i++) { A[i][k] *= inv_eta; sum += A[i][k] * A[i][k]; }
        double sigma = PNP_SQRT(sum);
        if (A[k][k] < 0) sigma = -sigma;
        A[k][k] += sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = (-eta) * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s = 0.0;
            for (int i = k; i < nr; i++) s += A[i][k] * A[i][j];
            const double tau = s / A1[k];
            for (int i = k; i < nr; i++) A[i][j] -= tau * A[i][k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0.0;
        for (int i = j; i < nr; i++) tau += A[i][j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i][j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double s = 0.0;
        for (int j = i + 1; j < nc; j++) s += A[i][j] * X[j];
        X[i] = (b[i] - s) / A2[i];
    }
    return true;
}

// gauss_newton (:812-858): five steps; READ: X starts as zeros (the reference's is uninitialised before its first solve)
PNP_HD void pnp_gauss_newton(const double* L, const double* rho, double* be)
{
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < 5; it++) {
        double A[6][4], b[6];
        for (int i = 0; i < 6; i++) {
            const double* r = L + 10 * i;
            A[i][0] = (((2 * r[0]) * be[0] + r[1] * be[1]) + r[3] * be[2]) + r[6] * be[3];
            A[i][1] = ((r[1] * be[0] + (2 * r[2]) * be[1]) + r[4] * be[2]) + r[7] * be[3];
            A[i][2] = ((r[3] * be[0] + r[4] * be[1]) + (2 * r[5]) * be[2]) + r[8] * be[3];
            A[i][3] = ((r[6] * be[0] + r[7] * be[1]) + r[8] * be[2]) + (2 * r[9]) * be[3];
            double q = (r[0] * be[0]) * be[0];
            q += (r[1] * be[0]) * be[1];
            q += (r[2] * be[1]) * be[1];
            q += (r[3] * be[0]) * be[2];
            q += (r[4] * be[1]) * be[2];
            q += (r[5] * be[2]) * be[2];
            q += (r[6] * be[0]) * be[3];
            q += (r[7] * be[1]) * be[3];
            q += (r[8] * be[2]) * be[3];
            q += (r[9] * be[3]) * be[3];
            b[i] = rho[i] - q;
        }
        pnp_qr_solve(A, b, x);
        for (int i = 0; i < 4; i++) be[i] += x[i];
    }
}

// fill_M's entry (row, col) of the 2n x 12 M
PNP_HD double pnp_M(const PnpPts& P, const PnpCam& C, int row, int col)
{
    const int i = row >> 1, k = col / 3, q = col - 3 * k;
    const double a = P.alphas[4 * i + k];
    if (row & 1) return q == 0 ? 0.0 : q == 1 ? a * C.fv : a * (C.vc - P.us[2 * i + 1]);
    return q == 0 ? a * C.fu : q == 1 ? 0.0 : a * (C.uc - P.us[2 * i]);
}

// compute_pose (:477-525) with everything it calls.  P.pws and P.us are filled and visible to every thread; the result is S.Rb, S.tb.
PNP_HD void pnp_compute_pose(PnpWork& S, const PnpPts& P, const PnpCam& C, int lane, int nth)
{
    const int n = P.n;
    const double nd = (double)n;
    PNP_BAR();
    // choose_control_points (:375-409)
    for (int e = lane; e < 3; e += nth) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s += P.pws[3 * i + e];
        S.cws[e] = s / nd;
    }
    PNP_BAR();
    for (int e = lane; e < 9; e += nth) {                             // cvMulTransposed(PW0, PW0tPW0, 1)
        const int r = e / 3, c = e - 3 * r;
        double s = 0.0;
        for (int i = 0; i < n; i++) s += (P.pws[3 * i + r] - S.cws[r]) * (P.pws[3 * i + c] - S.cws[c]);
        S.sA[e] = s;
    }
    pnp_svd(S.sA, 3, 3, nullptr, S.sW, lane, nth);
    if (lane == 0) {
        for (int i = 1; i < 4; i++) {
            const double k = PNP_SQRT(S.sW[i - 1] / nd);
            for (int j = 0; j < 3; j++) S.cws[3 * i + j] = S.cws[j] + k * S.sA[3 * (i - 1) + j];
        }
        // compute_barycentric_coordinates (:411-434): row j-1 of CC^T is cws[j] - cws[0]
        for (int j = 1; j < 4; j++)
            for (int i = 0; i < 3; i++) S.sA[3 * (j - 1) + i] = S.cws[3 * j + i] - S.cws[i];
    }
    pnp_svd(S.sA, 3, 3, S.sV, S.sW, lane, nth);
    if (lane == 0) {                                                  // cvInvert(CV_SVD): SVBkSb without a right-hand side
        double thr = ((0.0 + S.sW[0]) + S.sW[1]) + S.sW[2];
        thr *= PNP_DBL_EPSILON;
        for (int k = 0; k < 9; k++) S.ci[k] = 0.0;
        for (int i = 0; i < 3; i++) {
            double wi = S.sW[i];
            if (fabs(wi) <= thr) continue;
            wi = 1.0 / wi;
            double buf[3];
            for (int c = 0; c < 3; c++) buf[c] = S.sA[3 * i + c] * wi;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) S.ci[3 * r + c] = S.ci[3 * r + c] + S.sV[3 * i + r] * buf[c];
        }
    }
    PNP_BAR();
    for (int i = lane; i < n; i += nth) {
        const double* p = P.pws + 3 * i;
        double* a = P.alphas + 4 * i;
        for (int j = 0; j < 3; j++)
            a[1 + j] = (S.ci[3 * j] * (p[0] - S.cws[0]) + S.ci[3 * j + 1] * (p[1] - S.cws[1])) + S.ci[3 * j + 2] * (p[2] - S.cws[2]);
        a[0] = ((1.0 - a[1]) - a[2]) - a[3];
    }
    PNP_BAR();
    // cvMulTransposed(M, MtM, 1): each entry summed over M's rows in row order
    for (int e = lane; e < 144; e += nth) {
        const int r = e / 12, c = e - 12 * r;
        double s = 0.0;
        for (int row = 0; row < 2 * n; row++) s += pnp_M(P, C, row, r) * pnp_M(P, C, row, c);
        S.At[e] = s;
    }
    pnp_svd(S.At, 12, 12, nullptr, S.sW, lane, nth);
    if (lane == 0) {
        // compute_L_6x10 (:760-800), compute_rho (:802-810)
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        for (int i = 0; i < 6; i++) {
            double dv[4][3];
            for (int q = 0; q < 4; q++) {
                const double* v = S.At + 12 * (11 - q);
                for (int k = 0; k < 3; k++) dv[q][k] = v[3 * pa[i] + k] - v[3 * pb[i] + k];
            }
            double* row = S.L + 10 * i;
            row[0] = pnp_dot3(dv[0], dv[0]);
            row[1] = 2.0 * pnp_dot3(dv[0], dv[1]);
            row[2] = pnp_dot3(dv[1], dv[1]);
            row[3] = 2.0 * pnp_dot3(dv[0], dv[2]);
            row[4] = 2.0 * pnp_dot3(dv[1], dv[2]);
            row[5] = pnp_dot3(dv[2], dv[2]);
            row[6] = 2.0 * pnp_dot3(dv[0], dv[3]);
            row[7] = 2.0 * pnp_dot3(dv[1], dv[3]);
            row[8] = 2.0 * pnp_dot3(dv[2], dv[3]);
            row[9] = pnp_dot3(dv[3], dv[3]);
            S.rho[i] = pnp_dist2(S.cws + 3 * pa[i], S.cws + 3 * pb[i]);
        }
    }
    for (int which = 0; which < 3; which++) {
        // find_betas_approx_1 / 2 / 3 (:667-758): cvSolve(CV_SVD) on the chosen columns of L
        const int nc = which == 0 ? 4 : which == 1 ? 3 : 5;
        if (lane == 0) {
            const int cols[3][5] = {{0, 1, 3, 6, 0}, {0, 1, 2, 0, 0}, {0, 1, 2, 3, 4}};
            for (int c = 0; c < nc; c++)
                for (int r = 0; r < 6; r++) S.sA[6 * c + r] = S.L[10 * r + cols[which][c]];
        }
        pnp_svd(S.sA, 6, nc, S.sV, S.sW, lane, nth);
        if (lane == 0) {
            double thr = 0.0, b[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, be[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < nc; i++) thr += S.sW[i];
            thr *= PNP_DBL_EPSILON;
            for (int i = 0; i < nc; i++) {
                double wi = S.sW[i];
                if (fabs(wi) <= thr) continue;
                wi = 1.0 / wi;
                double s = 0.0;
                for (int j = 0; j < 6; j++) s += S.sA[6 * i + j] * S.rho[j];
                s *= wi;
                for (int j = 0; j < nc; j++) b[j] = b[j] + s * S.sV[nc * i + j];
            }
            if (which == 0) {
                if (b[0] < 0) { be[0] = PNP_SQRT(-b[0]); be[1] = -b[1] / be[0]; be[2] = -b[2] / be[0]; be[3] = -b[3] / be[0]; }
                else { be[0] = PNP_SQRT(b[0]); be[1] = b[1] / be[0]; be[2] = b[2] / be[0]; be[3] = b[3] / be[0]; }
            } else {
                if (b[0] < 0) { be[0] = PNP_SQRT(-b[0]); be[1] = b[2] < 0 ? PNP_SQRT(-b[2]) : 0.0; }
                else { be[0] = PNP_SQRT(b[0]); be[1] = b[2] > 0 ? PNP_SQRT(b[2]) : 0.0; }
                if (b[1] < 0) be[0] = -be[0];
                be[2] = which == 2 ? b[3] / be[0] : 0.0;
                be[3] = 0.0;
            }
            pnp_gauss_newton(S.L, S.rho, be);
            // compute_ccs (:453-464)
            for (int k = 0; k < 12; k++) S.ccs[k] = 0.0;
            for (int i = 0; i < 4; i++) {
                const double* v = S.At + 12 * (11 - i);
                for (int k = 0; k < 12; k++) S.ccs[k] += be[i] * v[k];
            }
        }
        PNP_BAR();
        // compute_pcs (:466-475)
        for (int i = lane; i < n; i += nth) {
            const double* a = P.alphas + 4 * i;
            for (int j = 0; j < 3; j++)
                P.pcs[3 * i + j] = ((a[0] * S.ccs[j] + a[1] * S.ccs[3 + j]) + a[2] * S.ccs[6 + j]) + a[3] * S.ccs[9 + j];
        }
        PNP_BAR();
        // solve_for_sign (:636-649): the depth of the FIRST correspondence decides
        const bool neg = n > 0 && P.pcs[2] < 0.0;
        PNP_BAR();
        if (neg) for (int i = lane; i < 3 * n; i += nth) P.pcs[i] = -P.pcs[i];
        PNP_BAR();
        // estimate_R_and_t (:569-627)
        for (int e = lane; e < 6; e += nth) {
            const double* src = e < 3 ? P.pcs + e : P.pws + (e - 3);
            double s = 0.0;
            for (int i = 0; i < n; i++) s += src[3 * i];
            if (e < 3) S.pc0[e] = s / nd; else S.pw0[e - 3] = s / nd;
        }
        PNP_BAR();
        for (int e = lane; e < 9; e += nth) {
            const int j = e / 3, c = e - 3 * j;
            double s = 0.0;
            for (int i = 0; i < n; i++) s += (P.pcs[3 * i + j] - S.pc0[j]) * (P.pws[3 * i + c] - S.pw0[c]);
            S.sA[3 * c + j] = s;                                      // the rows of ABt^T
        }
        pnp_svd(S.sA, 3, 3, S.sV, S.sW, lane, nth);
        if (lane == 0) {
            double* R = S.R[which];
            double* t = S.t[which];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {                         // dot(abt_u + 3*i, abt_v + 3*j): U[i][k] = Ut[k][i], V[j][k] = Vt[k][j]
                    R[3 * i + j] = (S.sA[i] * S.sV[j] + S.sA[3 + i] * S.sV[3 + j]) + S.sA[6 + i] * S.sV[6 + j];
                }
            double det = (R[0] * R[4]) * R[8] + (R[1] * R[5]) * R[6];
            det = det + (R[2] * R[3]) * R[7];
            det = det - (R[2] * R[4]) * R[6];
            det = det - (R[1] * R[3]) * R[8];
            det = det - (R[0] * R[5]) * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            for (int i = 0; i < 3; i++) t[i] = S.pc0[i] - pnp_dot3(R + 3 * i, S.pw0);
        }
        PNP_BAR();
        // reprojection_error (:550-567): the terms by correspondence, their sum in order
        {
            const double* R = S.R[which];
            const double* t = S.t[which];
            for (int i = lane; i < n; i += nth) {
                const double* pw = P.pws + 3 * i;
                const double Xc = pnp_dot3(R, pw) + t[0], Yc = pnp_dot3(R + 3, pw) + t[1];
                const double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
                const double ue = C.uc + (C.fu * Xc) * inv_Zc, ve = C.vc + (C.fv * Yc) * inv_Zc;
                const double u = P.us[2 * i], v = P.us[2 * i + 1];
                P.term[i] = PNP_SQRT((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
        }
        PNP_BAR();
        if (lane == 0) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s += P.term[i];
            S.err[which] = s / nd;
        }
        PNP_BAR();
    }
    if (lane == 0) {
        int N = 0;
        if (S.err[1] < S.err[0]) N = 1;
        if (S.err[2] < S.err[N]) N = 2;
        for (int k = 0; k < 9; k++) S.Rb[k] = S.R[N][k];
        for (int k = 0; k < 3; k++) S.tb[k] = S.t[N][k];
    }
    PNP_BAR();
}
