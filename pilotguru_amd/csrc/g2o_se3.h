// g2o_se3.h -- the pieces of g2o's SE3Quat (g2o/types/se3quat.h), of Eigen's quaternion and of RobustKernelHuber that the
// optimisers share (pose_opt.hip, local_ba.hip), in double and in the sources' operation order: DESIGN.md section 4 lists the readings.
#pragma once
#include <hip/hip_runtime.h>

struct PoSE3 { double qx, qy, qz, qw, tx, ty, tz; };

// SE3Quat::normalizeRotation: w < 0 flips every coefficient; then coeffs /= norm, the squared norm summed x, y, z, w
__device__ __forceinline__ void po_normalize(PoSE3& P)
{
    if (P.qw < 0.0) { P.qx *= -1.0; P.qy *= -1.0; P.qz *= -1.0; P.qw *= -1.0; }
    const double nrm = __dsqrt_rn(((P.qx * P.qx + P.qy * P.qy) + P.qz * P.qz) + P.qw * P.qw);
    P.qx /= nrm; P.qy /= nrm; P.qz /= nrm; P.qw /= nrm;
}

// Eigen's Quaterniond(Matrix3d); m row-major
__device__ __forceinline__ void po_quat_from_matrix(const double (&m)[9], PoSE3& P)
{
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = __dsqrt_rn(t + 1.0);
        P.qw = 0.5 * t;
        t = 0.5 / t;
        P.qx = (m[7] - m[5]) * t; P.qy = (m[2] - m[6]) * t; P.qz = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > (i ? m[4] : m[0])) i = 2;
        if (i == 0) {                                                   // j = 1, k = 2
            t = __dsqrt_rn(((m[0] - m[4]) - m[8]) + 1.0);
            P.qx = 0.5 * t; t = 0.5 / t;
            P.qw = (m[7] - m[5]) * t; P.qy = (m[3] + m[1]) * t; P.qz = (m[6] + m[2]) * t;
        } else if (i == 1) {                                            // j = 2, k = 0
            t = __dsqrt_rn(((m[4] - m[8]) - m[0]) + 1.0);
            P.qy = 0.5 * t; t = 0.5 / t;
            P.qw = (m[2] - m[6]) * t; P.qz = (m[7] + m[5]) * t; P.qx = (m[1] + m[3]) * t;
        } else {                                                        // j = 0, k = 1
            t = __dsqrt_rn(((m[8] - m[0]) - m[4]) + 1.0);
            P.qz = 0.5 * t; t = 0.5 / t;
            P.qw = (m[3] - m[1]) * t; P.qx = (m[2] + m[6]) * t; P.qy = (m[5] + m[7]) * t;
        }
    }
}

// Eigen's Quaternion::toRotationMatrix, row-major
__device__ __forceinline__ void po_matrix_from_quat(const PoSE3& P, double (&m)[9])
{
    const double tx = 2.0 * P.qx, ty = 2.0 * P.qy, tz = 2.0 * P.qz;
    const double twx = tx * P.qw, twy = ty * P.qw, twz = tz * P.qw, txx = tx * P.qx, txy = ty * P.qx, txz = tz * P.qx;
    const double tyy = ty * P.qy, tyz = tz * P.qy, tzz = tz * P.qz;
    m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy;
    m[3] = txy + twz; m[4] = 1.0 - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy; m[7] = tyz + twx; m[8] = 1.0 - (txx + tyy);
}

// Eigen's quaternion * vector: uv = vec x v; uv += uv; v + w * uv + vec x uv
__device__ __forceinline__ void po_rotate(const PoSE3& P, double X, double Y, double Z, double& rx, double& ry, double& rz)
{
    double ux = P.qy * Z - P.qz * Y, uy = P.qz * X - P.qx * Z, uz = P.qx * Y - P.qy * X;
    ux += ux; uy += uy; uz += uz;
    rx = (X + P.qw * ux) + (P.qy * uz - P.qz * uy);
    ry = (Y + P.qw * uy) + (P.qz * ux - P.qx * uz);
    rz = (Z + P.qw * uz) + (P.qx * uy - P.qy * ux);
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(update) * estimate (se3quat.h:223-257, :104-110); update = (omega, upsilon)
__device__ __forceinline__ PoSE3 po_oplus(const PoSE3& est, const double (&u)[6])
{
    const double o0 = u[0], o1 = u[1], o2 = u[2];
    const double theta = __dsqrt_rn((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9], R[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[r * 3 + c] = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
    if (theta < 0.00001) {
#pragma unroll
        for (int k = 0; k < 9; k++) { R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k]; V[k] = R[k]; }
    } else {
        const double s = sin(theta), c = cos(theta), t2 = theta * theta;
        const double a = s / theta, b = (1.0 - c) / t2, d = (theta - s) / (t2 * theta);      // pow(theta, 3) read as theta * theta * theta
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double I = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (I + a * Om[k]) + b * Om2[k];
            V[k] = (I + b * Om[k]) + d * Om2[k];
        }
    }
    PoSE3 E;
    po_quat_from_matrix(R, E);
    E.tx = (V[0] * u[3] + V[1] * u[4]) + V[2] * u[5];
    E.ty = (V[3] * u[3] + V[4] * u[4]) + V[5] * u[5];
    E.tz = (V[6] * u[3] + V[7] * u[4]) + V[8] * u[5];
    po_normalize(E);                                                    // SE3Quat(q, t)
    PoSE3 O;
    double rx, ry, rz;
    po_rotate(E, est.tx, est.ty, est.tz, rx, ry, rz);                   // result._t += _r * tr2._t
    O.tx = E.tx + rx; O.ty = E.ty + ry; O.tz = E.tz + rz;
    O.qw = ((E.qw * est.qw - E.qx * est.qx) - E.qy * est.qy) - E.qz * est.qz;       // result._r *= tr2._r
    O.qx = ((E.qw * est.qx + E.qx * est.qw) + E.qy * est.qz) - E.qz * est.qy;
    O.qy = ((E.qw * est.qy + E.qy * est.qw) + E.qz * est.qx) - E.qx * est.qz;
    O.qz = ((E.qw * est.qz + E.qz * est.qw) + E.qx * est.qy) - E.qy * est.qx;
    po_normalize(O);
    return O;
}

// chi2 = _error.dot(information * _error), information = invSigma2 * I
__device__ __forceinline__ double po_chi2(double e0, double e1, double w) { return e0 * (w * e0) + e1 * (w * e1); }

#define PO_DELTA ((double)0x1.394ca8p+1f)         /* (float)sqrt(5.991) = 2.4476519f */
// RobustKernelHuber::robustify: rho[0], rho[1]
__device__ __forceinline__ void po_huber(double e, double& rho0, double& rho1)
{
    const double dsqr = PO_DELTA * PO_DELTA;
    if (e <= dsqr) { rho0 = e; rho1 = 1.0; }
    else {
        const double sqrte = __dsqrt_rn(e);
        rho0 = 2.0 * sqrte * PO_DELTA - dsqr;
        rho1 = PO_DELTA / sqrte;
    }
}

__device__ __forceinline__ bool po_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for a NaN
