// g2o_se3.h -- g2o's SE3Quat (g2o/types/se3quat.h) and the SE3 edge and vertex pieces around it that the SE3 optimisers share
// (pose_opt.hip, local_ba.hip, global_ba.hip), each reading in ONE copy: normalizeRotation, VertexSE3Expmap's oplus, the reprojection
// error, EdgeSE3ProjectXYZ's linearisation, Converter::toSE3Quat, and toCvMat + SetPose (its Ow also serves loop_pose.h).  The
// quaternion, Huber and the solver pieces are g2o_lm.h's.  In double and in the sources' operation order: DESIGN.md section 4 lists
// the readings.
#pragma once
#include "match_common.h"
#include "g2o_lm.h"

struct PoSE3 { double qx, qy, qz, qw, tx, ty, tz; };

// Huber's delta of PoseOptimization and LocalBundleAdjustment (GlobalBundleAdjustemnt has its own float: GBA_DELTA)
#define PO_DELTA ((double)0x1.394ca8p+1f)         /* (float)sqrt(5.991) = 2.4476519f */

// SE3Quat::normalizeRotation: w < 0 flips every coefficient; then coeffs /= norm, the squared norm summed x, y, z, w
__device__ __forceinline__ void po_normalize(PoSE3& P)
{
    if (P.qw < 0.0) { P.qx *= -1.0; P.qy *= -1.0; P.qz *= -1.0; P.qw *= -1.0; }
    const double nrm = __dsqrt_rn(((P.qx * P.qx + P.qy * P.qy) + P.qz * P.qz) + P.qw * P.qw);
    P.qx /= nrm; P.qy /= nrm; P.qz /= nrm; P.qw /= nrm;
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
    g2o_quat_from_matrix(R, E);
    E.tx = (V[0] * u[3] + V[1] * u[4]) + V[2] * u[5];
    E.ty = (V[3] * u[3] + V[4] * u[4]) + V[5] * u[5];
    E.tz = (V[6] * u[3] + V[7] * u[4]) + V[8] * u[5];
    po_normalize(E);                                                    // SE3Quat(q, t)
    PoSE3 O;
    double rx, ry, rz;
    g2o_rotate(E, est.tx, est.ty, est.tz, rx, ry, rz);                   // result._t += _r * tr2._t
    O.tx = E.tx + rx; O.ty = E.ty + ry; O.tz = E.tz + rz;
    O.qw = ((E.qw * est.qw - E.qx * est.qx) - E.qy * est.qy) - E.qz * est.qz;       // result._r *= tr2._r
    O.qx = ((E.qw * est.qx + E.qx * est.qw) + E.qy * est.qz) - E.qz * est.qy;
    O.qy = ((E.qw * est.qy + E.qy * est.qw) + E.qz * est.qx) - E.qx * est.qz;
    O.qz = ((E.qw * est.qz + E.qz * est.qw) + E.qx * est.qy) - E.qy * est.qx;
    po_normalize(O);
    return O;
}

// computeError of EdgeSE3ProjectXYZ and EdgeSE3ProjectXYZOnlyPose: obs - cam_project(P.map(X)); (x, y, z) = the mapped point
__device__ __forceinline__ void po_error(const PoSE3& P, double fx, double fy, double cx, double cy, double X, double Y, double Z, double ox, double oy,
                                         double& x, double& y, double& z, double& e0, double& e1)
{
    double rx, ry, rz;
    g2o_rotate(P, X, Y, Z, rx, ry, rz);
    x = rx + P.tx; y = ry + P.ty; z = rz + P.tz;
    e0 = ox - ((x / z) * fx + cx);
    e1 = oy - ((y / z) * fy + cy);
}

// One EdgeSE3ProjectXYZ at the estimates (the bundle adjustments): the mapped point, the error, the robustified chi2,
// constructQuadraticForm's weights (base_binary_edge.hpp:60-116) and the pose Jacobian of linearizeOplus
// (types_six_dof_expmap.cpp:103-139), written as g2o writes it with x * y / z2.  EdgeSE3ProjectXYZOnlyPose's (:266-288) is written
// with invz and invz2 products, which round differently: it stays k_pose_opt's own.
struct PoLin { double x, y, z, e0, e1, rho0, wO, r0, r1, Jj0[6], Jj1[6]; };
__device__ __forceinline__ void po_linearize_xyz(const PoSE3& P, double fx, double fy, double cx, double cy, const double* X, double ox, double oy,
                                                 double wgt, bool robust, double delta, PoLin& L)
{
    po_error(P, fx, fy, cx, cy, X[0], X[1], X[2], ox, oy, L.x, L.y, L.z, L.e0, L.e1);
    const double x = L.x, y = L.y, z = L.z;
    const double c2 = g2o_chi2(L.e0, L.e1, wgt);
    double rho0 = c2, rho1 = 1.0;
    if (robust) g2o_huber(c2, delta, rho0, rho1);
    L.rho0 = rho0;
    const double z2 = z * z;
    const double Jj0[6] = {x * y / z2 * fx, -(1.0 + (x * x / z2)) * fx, y / z * fx, -1.0 / z * fx, 0.0, x / z2 * fx};
    const double Jj1[6] = {(1.0 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy, 0.0, -1.0 / z * fy, y / z2 * fy};
#pragma unroll
    for (int a = 0; a < 6; a++) { L.Jj0[a] = Jj0[a]; L.Jj1[a] = Jj1[a]; }
    // omega_r = -omega * _error (times rho[1]), weightedOmega = rho[1] * omega
    L.wO = rho1 * wgt; L.r0 = -(wgt * L.e0) * rho1; L.r1 = -(wgt * L.e1) * rho1;
}
// the point half of the same linearizeOplus: _jacobianOplusXi = -1./z * tmp * R
__device__ __forceinline__ void po_point_jacobian(const PoSE3& P, double fx, double fy, const PoLin& L, double (&Ji0)[3], double (&Ji1)[3])
{
    const double s = -1.0 / L.z;
    const double t0[3] = {s * fx, s * 0.0, s * (-L.x / L.z * fx)}, t1[3] = {s * 0.0, s * fy, s * (-L.y / L.z * fy)};
    double R[9];
    g2o_matrix_from_quat(P, R);
#pragma unroll
    for (int m = 0; m < 3; m++) {
        Ji0[m] = (t0[0] * R[m] + t0[1] * R[3 + m]) + t0[2] * R[6 + m];
        Ji1[m] = (t1[0] * R[m] + t1[1] * R[3 + m]) + t1[2] * R[6 + m];
    }
}

// Converter::toSE3Quat: SE3Quat(R, t) of the float Tcw
__device__ __forceinline__ PoSE3 po_from_pose(const pgorb_kf_pose& in)
{
    PoSE3 E;
    g2o_quat_from_pose(in.Tcw, E);
    E.tx = (double)in.Tcw[3]; E.ty = (double)in.Tcw[7]; E.tz = (double)in.Tcw[11];
    po_normalize(E);
    return E;
}

// Frame / KeyFrame::SetPose's Ow = -Rcw.t()*tcw of o.Tcw: gemm's small-matrix path times alpha = -1 in double
__device__ __forceinline__ void po_set_ow(pgorb_kf_pose& o)
{
#pragma unroll
    for (int c = 0; c < 3; c++)
        o.Ow[c] = cnm_f(__dmul_rn((double)cnm_dot3f(o.Tcw[c], o.Tcw[4 + c], o.Tcw[8 + c], o.Tcw[3], o.Tcw[7], o.Tcw[11]), -1.0));
}
// SetPose(Converter::toCvMat(SE3Quat)): Tcw as float, then Ow; the camera fields of o are kept
__device__ __forceinline__ void po_set_pose(const PoSE3& E, pgorb_kf_pose& o)
{
    double R[9];
    g2o_matrix_from_quat(E, R);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) o.Tcw[r * 4 + c] = __double2float_rn(R[r * 3 + c]);
    }
    o.Tcw[3] = __double2float_rn(E.tx); o.Tcw[7] = __double2float_rn(E.ty); o.Tcw[11] = __double2float_rn(E.tz);
    po_set_ow(o);
}
