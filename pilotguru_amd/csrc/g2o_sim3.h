// g2o_sim3.h -- g2o::Sim3 (g2o/types/sim3.h) as the Sim3 optimisers and loop closing share it (optimize_sim3.hip,
// essential_graph.hip, and through loop_pose.h loop_correct.hip, track_pose.hip and map_point.hip).  The quaternion under it is
// g2o_lm.h's, the same copy that g2o_se3.h uses.  In double and in the sources' operation order: DESIGN.md section 4 lists the readings.
#pragma once
#include "g2o_lm.h"

struct OsSim { double qx, qy, qz, qw, tx, ty, tz, s; };                 // g2o::Sim3: r (not renormalised), t, s

// Sim3::operator*: r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s; no renormalisation
__device__ __forceinline__ OsSim os_mul(const OsSim& a, const OsSim& b)
{
    OsSim O;
    double rx, ry, rz;
    O.qw = ((a.qw * b.qw - a.qx * b.qx) - a.qy * b.qy) - a.qz * b.qz;
    O.qx = ((a.qw * b.qx + a.qx * b.qw) + a.qy * b.qz) - a.qz * b.qy;
    O.qy = ((a.qw * b.qy + a.qy * b.qw) + a.qz * b.qx) - a.qx * b.qz;
    O.qz = ((a.qw * b.qz + a.qz * b.qw) + a.qx * b.qy) - a.qy * b.qx;
    g2o_rotate(a, b.tx, b.ty, b.tz, rx, ry, rz);
    O.tx = a.s * rx + a.tx; O.ty = a.s * ry + a.ty; O.tz = a.s * rz + a.tz;
    O.s = a.s * b.s;
    return O;
}

// Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1./s) * t), 1./s)
__device__ __forceinline__ OsSim os_inverse(const OsSim& a)
{
    OsSim O;
    const double k = -1.0 / a.s;
    O.qx = -a.qx; O.qy = -a.qy; O.qz = -a.qz; O.qw = a.qw;
    g2o_rotate(O, k * a.tx, k * a.ty, k * a.tz, O.tx, O.ty, O.tz);
    O.s = 1.0 / a.s;
    return O;
}

// Sim3(Vector7d) (sim3.h:70-142); update = (omega, upsilon, sigma)
__device__ __forceinline__ OsSim os_exp(const double (&u)[7])
{
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = __dsqrt_rn((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[r * 3 + c] = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
    OsSim E;
    E.s = exp(sigma);
    const double eps = 0.00001;
    double A, Bc, Cc;
    const bool smallTheta = theta < eps;
    if (smallTheta) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k];
    } else {
        const double a = sin(theta) / theta, b = (1.0 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * Om[k]) + b * Om2[k];
    }
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (smallTheta) { A = 1.0 / 2.0; Bc = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            Bc = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        Cc = (E.s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (smallTheta) {
            A = ((sigma - 1.0) * E.s + 1.0) / sigma2;
            Bc = (((0.5 * sigma2 - sigma) + 1.0) * E.s) / (sigma2 * sigma);
        } else {
            const double a = E.s * sin(theta), b = E.s * cos(theta), theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            Bc = (Cc - ((b - 1.0) * sigma + a * theta) / c) / theta2;
        }
    }
    g2o_quat_from_matrix(R, E);
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + Bc * Om2[k]) + Cc * (k % 4 == 0 ? 1.0 : 0.0);
    E.tx = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    E.ty = (W[3] * u[3] + W[4] * u[4]) + W[5] * u[5];
    E.tz = (W[6] * u[3] + W[7] * u[4]) + W[8] * u[5];
    return E;
}

// Sim3::log (sim3.h:148-230): (omega, upsilon, sigma).  deltaR is se3_ops.hpp's (R21 - R12, R02 - R20, R10 - R01); B*Omega*Omega is
// (B*Omega)*Omega; W.lu().solve(t) is read as Eigen's PartialPivLU of a 3 x 3: the first largest |entry| of a column pivots, the
// updates and both triangular solves run by columns.
__device__ __forceinline__ void os_log(const OsSim& P, double (&res)[7])
{
    const double sigma = log(P.s);
    double R[9];
    g2o_matrix_from_quat(P, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    const bool nearI = d > 1.0 - eps;
    double om[3], A, Bc, Cc, theta = 0.0;
    if (nearI) {
#pragma unroll
        for (int k = 0; k < 3; k++) om[k] = 0.5 * dR[k];
    } else {
        theta = acos(d);
        const double f = theta / (2.0 * __dsqrt_rn(1.0 - d * d));
#pragma unroll
        for (int k = 0; k < 3; k++) om[k] = f * dR[k];
    }
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (nearI) { A = 1.0 / 2.0; Bc = 1.0 / 6.0; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            Bc = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        Cc = (P.s - 1.0) / sigma;
        if (nearI) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * P.s + 1.0) / sigma2;
            Bc = (((0.5 * sigma2 - sigma) + 1.0) * P.s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta;
            const double a = P.s * sin(theta), b = P.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            Bc = ((Cc - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    const double Om[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    double W[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double bo2 = ((Bc * Om[r * 3]) * Om[c] + (Bc * Om[r * 3 + 1]) * Om[3 + c]) + (Bc * Om[r * 3 + 2]) * Om[6 + c];
            W[r * 3 + c] = (A * Om[r * 3 + c] + bo2) + Cc * (r == c ? 1.0 : 0.0);
        }
    // PartialPivLU, in place, and the solve on the permuted t
    double c3[3] = {P.tx, P.ty, P.tz};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int piv = k;
        double best = fabs(W[k * 3 + k]);
#pragma unroll
        for (int i = k + 1; i < 3; i++) { const double v = fabs(W[i * 3 + k]); if (v > best) { best = v; piv = i; } }
        if (piv != k) {
#pragma unroll
            for (int c = 0; c < 3; c++) { const double t = W[k * 3 + c]; W[k * 3 + c] = W[piv * 3 + c]; W[piv * 3 + c] = t; }
            const double t = c3[k]; c3[k] = c3[piv]; c3[piv] = t;
        }
        if (best != 0.0) {
#pragma unroll
            for (int i = k + 1; i < 3; i++) W[i * 3 + k] /= W[k * 3 + k];
        }
#pragma unroll
        for (int i = k + 1; i < 3; i++)
#pragma unroll
            for (int c = k + 1; c < 3; c++) W[i * 3 + c] -= W[i * 3 + k] * W[k * 3 + c];
    }
    c3[1] -= W[3] * c3[0]; c3[2] -= W[6] * c3[0]; c3[2] -= W[7] * c3[1];
    c3[2] /= W[8]; c3[0] -= W[2] * c3[2]; c3[1] -= W[5] * c3[2];
    c3[1] /= W[4]; c3[0] -= W[1] * c3[1];
    c3[0] /= W[0];
    res[0] = om[0]; res[1] = om[1]; res[2] = om[2]; res[3] = c3[0]; res[4] = c3[1]; res[5] = c3[2]; res[6] = sigma;
}
