// loop_pose.h -- the readings that loop correction (loop_correct.hip) shares with the essential graph (essential_graph.hip) and the
// map-point refresh (map_point.hip), each in ONE copy: Sim3::map, the [R | t/s] pose of a Sim3 with SetPose's Ow, the 4 x 4 pose
// product of cv::Mat, and the two pieces of MapPoint::UpdateNormalAndDepth.  DESIGN.md section 4 lists the readings.
#pragma once
#include "match_common.h"
#include "g2o_se3.h"                       // po_set_ow: SetPose's Ow
#include "g2o_sim3.h"

// Sim3::map: s*(r*xyz) + t
__device__ __forceinline__ void lp_map(const OsSim& S, double X, double Y, double Z, double& x, double& y, double& z)
{
    double rx, ry, rz;
    g2o_rotate(S, X, Y, Z, rx, ry, rz);
    x = S.s * rx + S.tx; y = S.s * ry + S.ty; z = S.s * rz + S.tz;
}

// [R | t/s] of a Sim3 (Optimizer.cc:1001-1007, LoopClosing.cc:504-510) through Converter::toCvSE3 to float, then SetPose's Ow; the
// camera fields of o are kept
__device__ __forceinline__ void lp_pose_from_sim3(const OsSim& S, pgorb_kf_pose& o)
{
    double R[9];
    g2o_matrix_from_quat(S, R);
    const double k = 1.0 / S.s;
    const double t[3] = {S.tx * k, S.ty * k, S.tz * k};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) o.Tcw[r * 4 + c] = __double2float_rn(R[r * 3 + c]);
        o.Tcw[r * 4 + 3] = __double2float_rn(t[r]);
    }
    po_set_ow(o);
}

// GetPoseInverse() of a pose as given: Twc = [Rcw' | Ow], rows 0-2
__device__ __forceinline__ void lp_twc(const pgorb_kf_pose& P, float (&T)[12])
{
#pragma unroll
    for (int r = 0; r < 3; r++) { T[r * 4] = P.Tcw[r]; T[r * 4 + 1] = P.Tcw[4 + r]; T[r * 4 + 2] = P.Tcw[8 + r]; T[r * 4 + 3] = P.Ow[r]; }
}

// rows 0-2 of the 4 x 4 float product A*B of two poses whose fourth rows are (0, 0, 0, 1): gemm's small-matrix path (len 4), the four
// terms in index order in float, the fourth term formed although its operand is the constant 0 or 1 (it decides the sign of a zero)
__device__ __forceinline__ void lp_mul44(const float* A, const float* B, float (&C)[12])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float s3 = __fadd_rn(__fadd_rn(__fmul_rn(A[r * 4], B[c]), __fmul_rn(A[r * 4 + 1], B[4 + c])), __fmul_rn(A[r * 4 + 2], B[8 + c]));
            C[r * 4 + c] = __fadd_rn(s3, __fmul_rn(A[r * 4 + 3], c == 3 ? 1.0f : 0.0f));
        }
}

// Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of the float pose rows T [12]
__device__ __forceinline__ OsSim lp_sim3_from_pose(const float* T)
{
    OsSim S;
    g2o_quat_from_pose(T, S);
    S.tx = (double)T[3]; S.ty = (double)T[7]; S.tz = (double)T[11]; S.s = 1.0;
    return S;
}

// one term of the normal: normali*(float)(1/cv::norm(normali)), normali = mWorldPos - Ow (MapPoint.cc:370-372); nd = cv::norm(normali)
__device__ __forceinline__ void mp_term(const float* pos, const float* Ow, float t[3], double& nd)
{
    const float x = __fsub_rn(pos[0], Ow[0]), y = __fsub_rn(pos[1], Ow[1]), z = __fsub_rn(pos[2], Ow[2]);
    nd = cnm_normd(x, y, z);
    const float sc = cnm_f(__ddiv_rn(1.0, nd));
    t[0] = __fmul_rn(x, sc); t[1] = __fmul_rn(y, sc); t[2] = __fmul_rn(z, sc);
}
// mfMaxDistance, mfMinDistance from dist = cv::norm(Pos - Ow_ref) and the reference keypoint's octave (:376-385); sf = mvScaleFactors
__device__ __forceinline__ void mp_depth(const float* sf, int nlevels, double nd, int octave, float& minD, float& maxD)
{
    const int level = min((unsigned)octave, (unsigned)PG_MAXL);
    maxD = __fmul_rn(cnm_f(nd), sf[level]);
    minD = __fdiv_rn(maxD, sf[max(nlevels - 1, 0)]);
}
