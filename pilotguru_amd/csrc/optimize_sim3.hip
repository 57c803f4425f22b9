// optimize_sim3.hip -- Optimizer::OptimizeSim3 on gfx950: the refinement of a loop candidate's Sim3 over its matched map points, one
// workgroup per key-frame pair and one launch per call.
//
// Restates (thirdparty/orb-slam2, thirdparty/g2o):
//   Optimizer::OptimizeSim3                       src/Optimizer.cc:1046-1241
//   LoopClosing::ComputeSim3                      src/LoopClosing.cc:320-335 (gScm from the float R, t, s; gScm*gSmw; toCvMat)
//   Sim3 (Sim3(Vector7d), map, inverse, operator*)   g2o/types/sim3.h:59-142, :144-146, :233-236, :266-272
//   VertexSim3Expmap::oplusImpl, cam_map1 / 2     g2o/types/types_seven_dof_expmap.h:60-88
//   EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError   :138-167 (both linearizeOplus overrides are commented out)
//   BaseBinaryEdge::linearizeOplus                g2o/core/base_binary_edge.hpp:131-205 (central differences, delta = 1e-9)
//   BaseBinaryEdge::constructQuadraticForm        :55-120, RobustKernelHuber::robustify robust_kernel_impl.cpp:78-91
//   OptimizationAlgorithmLevenberg::solve         g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   LinearSolverDense::solve                      g2o/solvers/linear_solver_dense.h:104-112
// in double, in the reference's operation order per edge, under the readings of DESIGN.md section 4 (the OptimizeSim3 rows).  This is
// the project's reading of g2o and Eigen, anchored by the CPU tests of tests/test_optimize_sim3.py and not pinned to a g2o build.
// Shared, each in one copy: Huber, the LDLT, Levenberg's step control, the block reductions and the quaternion are g2o_lm.h's (with
// pose_opt.hip, local_ba.hip, essential_graph.hip, global_ba.hip); Sim3 is g2o_sim3.h's (with essential_graph.hip and loop_pose.h);
// SetPose's Ow is g2o_se3.h's.  This file's own: the two edges' computeError through Sim3::map and the numeric Jacobian.
//
// k_optimize_sim3, OS_T threads:
//   1. the correspondences (a match whose two slots hold good points) are compacted in i1 order by ballot prefix into 64-byte records
//      (P1c, P2c, the two observations, the two invSigma2, i1, i2, removed) in the context's scratch arena;
//   2. per linearisation the 14 estimates Sim3(+-1e-9 e_d) * estimate and their inverses are formed once, by lanes 0-13, and kept in
//      LDS; correspondence e belongs to lane e mod OS_T, which takes both of its edges (e12 first) against them: the numeric Jacobian;
//   3. a lane sums its correspondences in increasing e into 36 doubles (the 28 upper entries of H, b, chi2), reduced by a butterfly
//      inside each wave and then as (w0 + w1) + (w2 + w3) through LDS -- one fixed tree, so a pair's result depends on its inputs alone;
//   4. the Levenberg state is carried identically by every lane.  Every loop is bounded by 2 calls x 10 iterations x 10 trials.
#include "kf_window.h"
#include "g2o_se3.h"                        // po_set_ow: SetPose's Ow
#include "g2o_sim3.h"
#include <math.h>
#include <string>

#define OS_T 256
#define OS_WAVES (OS_T / 64)
#define OS_MAX_N 16000            // keypoints per key frame, as for the matchers
#define OS_NRED 36                // 28 + 7 + 1

struct OsRec { float P1[3], P2[3], o1[2], o2[2], w1, w2; int32_t i1, i2, dead, pad; };
static_assert(sizeof(OsRec) == 64, "four dwordx4");

struct OsBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap; const int32_t* pairKF1; const int32_t* pairKF2; const pgorb_kf_pose* pose;
    const int32_t* kfPoint; const int32_t* matches12; const int32_t* newMatches12; int npoints; const pgorb_map_point* pts; const uint8_t* pbad;
    int nlevels; float invSigma2[PG_MAXL + 1];
    const pgorb_sim3_estimate* est; double th2, delta; int fixScale;
    OsRec* recs;
    pgorb_sim3_estimate* estOut; int32_t* matchesOut; float* chi12; float* chi21; pgorb_kf_pose* scwPose; int32_t* info; int32_t* nIn;
};

struct OsCam { double fx, fy, cx, cy; };

// computeError of either edge: obs - cam_map(project(S.map(X))); for EdgeInverseSim3ProjectXYZ S is the inverse
__device__ __forceinline__ void os_error(const OsSim& S, const OsCam& C, double X, double Y, double Z, double ox, double oy, double& e0, double& e1)
{
    double rx, ry, rz;
    g2o_rotate(S, X, Y, Z, rx, ry, rz);
    const double x = S.s * rx + S.tx, y = S.s * ry + S.ty, z = S.s * rz + S.tz;
    e0 = ox - ((x / z) * C.fx + C.cx);
    e1 = oy - ((y / z) * C.fy + C.cy);
}
__device__ __forceinline__ OsRec os_load(const OsRec* r)
{
    const float4* s = reinterpret_cast<const float4*>(r);
    const float4 a = s[0], b = s[1], c = s[2], d = s[3];
    OsRec R;
    R.P1[0] = a.x; R.P1[1] = a.y; R.P1[2] = a.z; R.P2[0] = a.w; R.P2[1] = b.x; R.P2[2] = b.y;
    R.o1[0] = b.z; R.o1[1] = b.w; R.o2[0] = c.x; R.o2[1] = c.y; R.w1 = c.z; R.w2 = c.w;
    R.i1 = __float_as_int(d.x); R.i2 = __float_as_int(d.y); R.dead = __float_as_int(d.z); R.pad = 0;
    return R;
}

struct OsShared {
    OsSim pert[14], pinv[14];             // Sim3(+delta e_d) * estimate at 2d, Sim3(-delta e_d) * estimate at 2d + 1, and their inverses
    double part[OS_WAVES][OS_NRED];       // part[0][0 .. 3] also serve the scalar sums
    double red[OS_NRED];
    int cnt[OS_WAVES];
};

// One edge into the lane's sums: computeError at the estimate, the numeric Jacobian against the 14 perturbed estimates of LDS
// (INV: their inverses), constructQuadraticForm with the Huber kernel
template <bool INV>
__device__ __forceinline__ void os_edge(const OsShared& S, const OsSim& at, const OsCam& C, double X, double Y, double Z, double ox, double oy, double w,
                                        double delta, double (&acc)[OS_NRED])
{
    double e0, e1;
    os_error(at, C, X, Y, Z, ox, oy, e0, e1);
    const double c2 = g2o_chi2(e0, e1, w);
    double rho0, rho1;
    g2o_huber(c2, delta, rho0, rho1);
    const double scalar = 1.0 / (2.0 * 1e-9);
    double J0[7], J1[7];
    // The 28 estimates do not change inside the caller's loop, so the compiler would read them all ahead of it and hold 448 VGPRs
    // across it.  `off` is always 0, but opaque and produced only after the previous column: one pair of estimates is live at a time.
    int off = 0;
#pragma unroll
    for (int d = 0; d < 7; d++) {
        const OsSim Sp = INV ? S.pinv[2 * d + off] : S.pert[2 * d + off];
        const OsSim Sm = INV ? S.pinv[2 * d + 1 + off] : S.pert[2 * d + 1 + off];
        double p0, p1, m0, m1;
        os_error(Sp, C, X, Y, Z, ox, oy, p0, p1);
        os_error(Sm, C, X, Y, Z, ox, oy, m0, m1);
        J0[d] = scalar * (p0 - m0);
        J1[d] = scalar * (p1 - m1);
        asm volatile("" : "+v"(off) : "v"(J0[d]), "v"(J1[d]));
    }
    // omega_r = -(omega * e) * rho1; b += B' * omega_r; H += (B' * (rho1 * omega)) * B
    const double wr = rho1 * w, r0 = (-(w * e0)) * rho1, r1 = (-(w * e1)) * rho1;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const double a0 = J0[i] * wr, a1 = J1[i] * wr;
#pragma unroll
        for (int j = i; j < 7; j++) acc[k++] += a0 * J0[j] + a1 * J1[j];
    }
#pragma unroll
    for (int i = 0; i < 7; i++) acc[28 + i] += J0[i] * r0 + J1[i] * r1;
    acc[35] += rho0;
}

// activeRobustChi2 at P over the lane's remaining correspondences
__device__ __forceinline__ double os_active_chi2(OsShared& S, const OsRec* E, int nE, const OsSim& P, const OsCam& C1, const OsCam& C2, double delta)
{
    const OsSim Pi = os_inverse(P);
    double acc = 0.0;
    for (int e = threadIdx.x; e < nE; e += OS_T) {
        const OsRec r = os_load(E + e);
        if (r.dead) continue;
        double e0, e1, r0, r1;
        os_error(P, C1, (double)r.P2[0], (double)r.P2[1], (double)r.P2[2], (double)r.o1[0], (double)r.o1[1], e0, e1);
        g2o_huber(g2o_chi2(e0, e1, (double)r.w1), delta, r0, r1);
        acc += r0;
        os_error(Pi, C2, (double)r.P1[0], (double)r.P1[1], (double)r.P1[2], (double)r.o2[0], (double)r.o2[1], e0, e1);
        g2o_huber(g2o_chi2(e0, e1, (double)r.w2), delta, r0, r1);
        acc += r0;
    }
    return g2o_block_sum(S.part[0], acc);
}

__global__ __launch_bounds__(OS_T) void k_optimize_sim3(OsBatch B)
{
    __shared__ OsShared S;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f1 = B.pairKF1 ? B.pairKF1[p] : 0, f2 = B.pairKF2 ? B.pairKF2[p] : 1;
    const int n1 = min(max(B.n[f1], 0), B.cap), n2 = min(max(B.n[f2], 0), B.cap);
    const int64_t row = (int64_t)p * B.cap;
    const pgorb_keypoint* K1 = B.K + (int64_t)f1 * B.cap;
    const pgorb_keypoint* K2 = B.K + (int64_t)f2 * B.cap;
    const int32_t* S1 = B.kfPoint + (int64_t)f1 * B.cap;
    const int32_t* S2 = B.kfPoint + (int64_t)f2 * B.cap;
    const pgorb_kf_pose P1 = B.pose[f1], P2 = B.pose[f2];
    OsRec* E = B.recs + row;

    // 1. the correspondences, in i1 order (Optimizer.cc:1099-1178); new_matches12 replaces an entry where it is >= 0
    int nE = 0;
    for (int i0 = 0; i0 < B.cap; i0 += OS_T) {
        const int i1 = i0 + tid;
        int m = -1;
        if (i1 < n1) {
            m = B.matches12[row + i1];
            if (B.newMatches12) { const int nm = B.newMatches12[row + i1]; if (nm >= 0) m = nm; }
        }
        int i2 = (m >= 0 && m < n2) ? m : -1;
        int s1 = -1, s2 = -1;
        pgorb_keypoint k1, k2;
        if (i2 >= 0) {
            s1 = S1[i1]; s2 = S2[i2];
            if (s1 < 0 || s1 >= B.npoints || s2 < 0 || s2 >= B.npoints) i2 = -1;
        }
        if (i2 >= 0 && B.pbad && (B.pbad[s1] | B.pbad[s2])) i2 = -1;
        if (i2 >= 0) {
            k1 = K1[i1]; k2 = K2[i2];
            if (k1.octave < 0 || k1.octave >= B.nlevels || k2.octave < 0 || k2.octave >= B.nlevels) i2 = -1;
        }
        const unsigned long long bm = __ballot(i2 >= 0);
        if (lane == 0) S.cnt[wave] = __popcll(bm);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < OS_WAVES; w++) { const int c = S.cnt[w]; if (w < wave) before += c; total += c; }
        __syncthreads();
        if (i2 >= 0) {
            const int e = nE + before + __popcll(bm & ((1ull << lane) - 1ull));
            float X1[3], X2[3];
            kf_to_camera(P1, B.pts[s1].pos, X1);                        // P3D1c = R1w*P3D1w + t1w
            kf_to_camera(P2, B.pts[s2].pos, X2);
            float4* dst = reinterpret_cast<float4*>(E + e);
            dst[0] = make_float4(X1[0], X1[1], X1[2], X2[0]);
            dst[1] = make_float4(X2[1], X2[2], k1.x, k1.y);
            dst[2] = make_float4(k2.x, k2.y, B.invSigma2[k1.octave], B.invSigma2[k2.octave]);
            dst[3] = make_float4(__int_as_float(i1), __int_as_float(i2), __int_as_float(0), __int_as_float(0));
        }
        if (i1 < B.cap) {
            B.matchesOut[row + i1] = m;
            if (B.chi12) B.chi12[row + i1] = 0.0f;
            if (B.chi21) B.chi21[row + i1] = 0.0f;
        }
        nE += total;
    }
    __syncthreads();                                                    // a record is written by its keypoint's lane and read by its owner, lane e mod OS_T

    const OsCam C1 = {(double)P1.fx, (double)P1.fy, (double)P1.cx, (double)P1.cy};
    const OsCam C2 = {(double)P2.fx, (double)P2.fy, (double)P2.cx, (double)P2.cy};
    const pgorb_sim3_estimate in = B.est[p];
    // g2o::Sim3 gScm(Converter::toMatrix3d(R), Converter::toVector3d(t), s) (LoopClosing.cc:325)
    OsSim est;
    {
        double R[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (double)in.R12[k];
        g2o_quat_from_matrix(R, est);
        est.tx = (double)in.t12[0]; est.ty = (double)in.t12[1]; est.tz = (double)in.t12[2]; est.s = (double)in.s12;
    }

    int status = 0, nBad = 0, nIn = 0, nMore = 0;
    int its[2] = {0, 0}, trials[2] = {0, 0};
    OsSim errEst = est;                                                 // where the active edges' _error was last computed
    for (int call = 0; call < 2 && !status; call++) {
        const int iterations = call == 0 ? 5 : nMore;
        // SparseOptimizer::optimize(iterations); an empty active set returns at once
        if (nE - nBad > 0) {
            G2oLm lm = {0.0, 2, 0};
            for (int iter = 0; iter < iterations; iter++) {
                // linearizeOplus' perturbed estimates: oplus(+-delta e_d); under fix_scale oplusImpl zeroes add_vi[6]
                if (tid < 14) {
                    const int d = tid >> 1;
                    const double v = (tid & 1) ? -1e-9 : 1e-9;
                    double u[7];
#pragma unroll
                    for (int k = 0; k < 7; k++) u[k] = k == d ? v : 0.0;
                    if (B.fixScale) u[6] = 0.0;
                    const OsSim Pt = os_mul(os_exp(u), est);
                    S.pert[tid] = Pt;
                    S.pinv[tid] = os_inverse(Pt);
                }
                __syncthreads();
                // computeActiveErrors, activeRobustChi2, buildSystem
                const OsSim estInv = os_inverse(est);
                double acc[OS_NRED];
#pragma unroll
                for (int k = 0; k < OS_NRED; k++) acc[k] = 0.0;
#pragma unroll 1
                for (int e = tid; e < nE; e += OS_T) {
                    const OsRec r = os_load(E + e);
                    if (r.dead) continue;
                    os_edge<false>(S, est, C1, (double)r.P2[0], (double)r.P2[1], (double)r.P2[2], (double)r.o1[0], (double)r.o1[1], (double)r.w1, B.delta, acc);
                    os_edge<true>(S, estInv, C2, (double)r.P1[0], (double)r.P1[1], (double)r.P1[2], (double)r.o2[0], (double)r.o2[1], (double)r.w2, B.delta, acc);
                }
                g2o_block_sum_n(S.part, S.red, acc);
                double H[7][7], b[7];
                g2o_dense_system(S.red, H, b);
                double currentChi = S.red[35];
                const double iniChi = currentChi;
                if (!g2o_finite(currentChi)) { status = PGORB_OS3_NONFINITE; break; }
                if (iter == 0) g2o_lm_begin(lm, g2o_lm_lambda_init(g2o_max_diagonal(H)));
                its[call]++;
                double rho = 0.0;
                int qmax = 0;
                do {
                    double x[7], scale;
                    const bool ok2 = g2o_dense_trial(H, b, lm.lambda, B.fixScale != 0, x, scale);
                    const OsSim trial = os_mul(os_exp(x), est);
                    errEst = trial;
                    const double tempChi = os_active_chi2(S, E, nE, trial, C1, C2, B.delta);
                    if (g2o_lm_decide(lm, currentChi, tempChi, ok2, scale, rho)) est = trial;       // discardTop; else pop
                    qmax++; trials[call]++;
                } while (g2o_lm_again(rho, qmax));
                if (g2o_lm_stop(lm, iniChi, currentChi, qmax, rho)) break;
            }
        }
        if (status) break;
        // the classification (:1186-1203, :1220-1234): e->chi2() of the errors the last trial left, no computeError
        const OsSim errInv = os_inverse(errEst);
        int bad = 0, good = 0, nonfinite = 0;
        for (int e = tid; e < nE; e += OS_T) {
            const OsRec r = os_load(E + e);
            if (r.dead) continue;
            double e0, e1;
            os_error(errEst, C1, (double)r.P2[0], (double)r.P2[1], (double)r.P2[2], (double)r.o1[0], (double)r.o1[1], e0, e1);
            const double c12 = g2o_chi2(e0, e1, (double)r.w1);
            os_error(errInv, C2, (double)r.P1[0], (double)r.P1[1], (double)r.P1[2], (double)r.o2[0], (double)r.o2[1], e0, e1);
            const double c21 = g2o_chi2(e0, e1, (double)r.w2);
            if (!g2o_finite(c12) || !g2o_finite(c21)) nonfinite = 1;
            const int out = (c12 > B.th2 || c21 > B.th2) ? 1 : 0;
            bad += out; good += 1 - out;
            if (out) { B.matchesOut[row + r.i1] = -1; if (call == 0) E[e].dead = 1; }
            if (B.chi12) B.chi12[row + r.i1] = __double2float_rn(c12);
            if (B.chi21) B.chi21[row + r.i1] = __double2float_rn(c21);
        }
        if (__syncthreads_or(nonfinite)) { status = PGORB_OS3_NONFINITE; break; }
        if (call == 0) {
            nBad = g2o_block_sum(S.cnt, bad);
            nMore = nBad > 0 ? 10 : 5;
            if (nE - nBad < 10) status = PGORB_OS3_FEW;                 // return 0 before the vertex is recovered (:1211)
        } else {
            nIn = g2o_block_sum(S.cnt, good);
        }
    }

    if (status & PGORB_OS3_NONFINITE) {                                 // nothing is removed, no chi2 is reported
        for (int e = tid; e < nE; e += OS_T) {
            const OsRec r = os_load(E + e);
            B.matchesOut[row + r.i1] = r.i2;
            if (B.chi12) B.chi12[row + r.i1] = 0.0f;
            if (B.chi21) B.chi21[row + r.i1] = 0.0f;
        }
    }
    if (tid == 0) {
        pgorb_sim3_estimate o = in;
        pgorb_kf_pose sp;
        memset(&sp, 0, sizeof(sp));
        if (!status) {
            double R[9];
            g2o_matrix_from_quat(est, R);
#pragma unroll
            for (int k = 0; k < 9; k++) o.R12[k] = __double2float_rn(R[k]);
            o.t12[0] = __double2float_rn(est.tx); o.t12[1] = __double2float_rn(est.ty); o.t12[2] = __double2float_rn(est.tz);
            o.s12 = __double2float_rn(est.s);
            // mg2oScw = gScm * gSmw, gSmw = Sim3(toMatrix3d(R2w), toVector3d(t2w), 1.0); mScw = toCvMat: s * R and t as float
            OsSim mw;
            g2o_quat_from_pose(P2.Tcw, mw);
            mw.tx = (double)P2.Tcw[3]; mw.ty = (double)P2.Tcw[7]; mw.tz = (double)P2.Tcw[11]; mw.s = 1.0;
            const OsSim cw = os_mul(est, mw);
            g2o_matrix_from_quat(cw, R);
            float sR[9], st[3] = {__double2float_rn(cw.tx), __double2float_rn(cw.ty), __double2float_rn(cw.tz)};
#pragma unroll
            for (int k = 0; k < 9; k++) sR[k] = __double2float_rn(cw.s * R[k]);
            // ORBmatcher.cc:301-305: scw = sqrt(sRcw.row(0).dot(sRcw.row(0))), Rcw = sRcw/scw, tcw = Scw.col(3)/scw, Ow = -Rcw.t()*tcw
            const float scw = cnm_f(cnm_normd(sR[0], sR[1], sR[2]));
            const float a = cnm_f(__ddiv_rn(1.0, (double)scw));
            sp = P1;                                                    // KF1's camera
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) sp.Tcw[r * 4 + c] = __fmul_rn(sR[r * 3 + c], a);
                sp.Tcw[r * 4 + 3] = __fmul_rn(st[r], a);
            }
            po_set_ow(sp);
        }
        B.estOut[p] = o;
        if (B.scwPose) B.scwPose[p] = sp;
        if (B.nIn) B.nIn[p] = status ? 0 : nIn;
        if (B.info) {
            int32_t* I = B.info + (int64_t)p * PGORB_OS3_INFO;
            I[0] = status; I[1] = nE; I[2] = nBad; I[3] = its[0]; I[4] = trials[0]; I[5] = its[1]; I[6] = trials[1]; I[7] = nMore;
        }
    }
}

extern "C" {

int pgorb_optimize_sim3_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap, const int32_t* d_pair_kf1,
        const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, const int32_t* d_kf_point, const int32_t* d_matches12,
        const int32_t* d_new_matches12, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_bad,
        const pgorb_sim3_estimate* d_estimate, float th2, int fix_scale, pgorb_sim3_estimate* d_estimate_out, int32_t* d_matches12_out,
        float* d_chi2_12, float* d_chi2_21, pgorb_kf_pose* d_scw_pose, int32_t* d_info, int32_t* d_nin, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || cap < 1 || npairs < 0 || npoints < 0 || !(th2 > 0.0f) || !std::isfinite(th2) ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_pose || !d_kf_point || !d_matches12 || !d_estimate || !d_estimate_out || !d_matches12_out)) ||
        (npoints && !d_points))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_optimize_sim3_batch_device");
    if (cap > OS_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_sim3: more than 16000 keypoints per frame");
    if (!npairs) return 0;
    OsBatch B;
    B.nlevels = pgorb_levels(c);
    memset(B.invSigma2, 0, sizeof(B.invSigma2));
    if (!(B.nlevels > 0) || B.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, nullptr, B.invSigma2) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    hipStream_t s = (hipStream_t)stream;
    void* scr;
    int rc = pg_ctx_scratch(c, (size_t)npairs * cap * sizeof(OsRec), s, &scr);
    if (rc) return rc;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.pairKF1 = d_pair_kf1; B.pairKF2 = d_pair_kf2; B.pose = d_pose; B.kfPoint = d_kf_point;
    B.matches12 = d_matches12; B.newMatches12 = d_new_matches12; B.npoints = npoints; B.pts = d_points; B.pbad = d_point_bad;
    B.est = d_estimate; B.th2 = (double)th2; B.delta = (double)(float)sqrt((double)th2);      // const float deltaHuber = sqrt(th2)
    B.fixScale = fix_scale ? 1 : 0; B.recs = (OsRec*)scr;
    B.estOut = d_estimate_out; B.matchesOut = d_matches12_out; B.chi12 = d_chi2_12; B.chi21 = d_chi2_21; B.scwPose = d_scw_pose;
    B.info = d_info; B.nIn = d_nin;
    hipLaunchKernelGGL(k_optimize_sim3, dim3((unsigned)npairs), dim3(OS_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_optimize_sim3 launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool os_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

int pgorb_optimize_sim3(pgorb_ctx* c, const pgorb_keypoint* kps1, int n1, const pgorb_kf_pose* pose1, const int32_t* kf_point1,
        const pgorb_keypoint* kps2, int n2, const pgorb_kf_pose* pose2, const int32_t* kf_point2, const int32_t* matches12,
        const int32_t* new_matches12, int npoints, const pgorb_map_point* points, const uint8_t* point_bad,
        const pgorb_sim3_estimate* estimate, float th2, int fix_scale, pgorb_sim3_estimate* estimate_out, int32_t* matches12_out,
        float* chi2_12, float* chi2_21, pgorb_kf_pose* scw_pose, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    if (n1 < 0 || n2 < 0 || npoints < 0) why = "a count is negative";
    else if (!pose1 || !pose2 || !estimate || !estimate_out || (n1 && (!kps1 || !kf_point1 || !matches12 || !matches12_out)) ||
             (n2 && (!kps2 || !kf_point2)) || (npoints && !points)) why = "an array that is read is NULL";
    else if (!os_all_finite(pose1->Tcw, 12) || !os_all_finite(&pose1->fx, 4) || !os_all_finite(pose2->Tcw, 12) || !os_all_finite(&pose2->fx, 4))
        why = "a pose or a camera is not finite";
    else if (!os_all_finite(estimate->R12, 13)) why = "the estimate is not finite";
    else if (!(estimate->s12 > 0.0f)) why = "the estimate's scale is not positive";
    else if (!(th2 > 0.0f) || !std::isfinite(th2)) why = "th2 is not positive";
    for (int i = 0; !why && i < n1; i++)
        if (kf_point1[i] < -1 || kf_point1[i] >= npoints) why = "a slot's point index is out of range";
    for (int i = 0; !why && i < n2; i++)
        if (kf_point2[i] < -1 || kf_point2[i] >= npoints) why = "a slot's point index is out of range";
    for (int i = 0; !why && i < n1; i++) {
        if (matches12[i] < -1 || matches12[i] >= n2) { why = "matches12 is outside [-1, n2)"; break; }
        if (new_matches12 && (new_matches12[i] < -1 || new_matches12[i] >= n2)) { why = "new_matches12 is outside [-1, n2)"; break; }
        const int j = (new_matches12 && new_matches12[i] >= 0) ? new_matches12[i] : matches12[i];
        if (j < 0 || kf_point1[i] < 0 || kf_point2[j] < 0) continue;
        if (kps1[i].octave < 0 || kps1[i].octave >= nlevels || kps2[j].octave < 0 || kps2[j].octave >= nlevels) why = "an octave is outside the context's levels";
        else if (!os_all_finite(points[kf_point1[i]].pos, 3) || !os_all_finite(points[kf_point2[j]].pos, 3)) why = "a referenced point is not finite";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_optimize_sim3: ") + why).c_str());
    if (n1 > OS_MAX_N || n2 > OS_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_sim3: more than 16000 keypoints per frame");
    const int cap = std::max(std::max(n1, n2), 1), np = std::max(npoints, 1);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)2 * cap * sizeof(pgorb_keypoint)), oPose = s.region(PG_UP, 2 * sizeof(pgorb_kf_pose)),
                 oS = s.region(PG_UP, (size_t)2 * cap * 4), oM = s.region(PG_UP, (size_t)cap * 4), oNM = s.region(PG_UP, new_matches12 ? (size_t)cap * 4 : 0),
                 oP = s.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)), oB = s.region(PG_UP, point_bad ? np : 0),
                 oE = s.region(PG_UP, sizeof(pgorb_sim3_estimate)),
                 oEO = s.region(PG_DOWN, sizeof(pgorb_sim3_estimate)), oMO = s.region(PG_DOWN, (size_t)cap * 4), oC1 = s.region(PG_DOWN, (size_t)cap * 4),
                 oC2 = s.region(PG_DOWN, (size_t)cap * 4), oSP = s.region(PG_DOWN, sizeof(pgorb_kf_pose)), oR = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t cnt[4] = {n1, n2, 0, 1};                              // n of frames 0 and 1, then the pair (0, 1)
    s.put(oN, cnt, 16);
    s.put(oK, kps1, (size_t)n1 * sizeof(pgorb_keypoint), 0, (size_t)cap * sizeof(pgorb_keypoint));
    s.put(oK, kps2, (size_t)n2 * sizeof(pgorb_keypoint), (size_t)cap * sizeof(pgorb_keypoint), (size_t)cap * sizeof(pgorb_keypoint));
    s.put(oPose, pose1, sizeof(pgorb_kf_pose));
    s.put(oPose, pose2, sizeof(pgorb_kf_pose), sizeof(pgorb_kf_pose));
    memset(s.host(oS), 0xFF, (size_t)2 * cap * 4);
    s.put(oS, kf_point1, (size_t)n1 * 4);
    s.put(oS, kf_point2, (size_t)n2 * 4, (size_t)cap * 4);
    memset(s.host(oM), 0xFF, (size_t)cap * 4);
    s.put(oM, matches12, (size_t)n1 * 4);
    if (new_matches12) { memset(s.host(oNM), 0xFF, (size_t)cap * 4); s.put(oNM, new_matches12, (size_t)n1 * 4); }
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    if (point_bad) s.put(oB, point_bad, npoints, 0, np);
    s.put(oE, estimate, sizeof(pgorb_sim3_estimate));
    int32_t* R = s.dev<int32_t>(oR);                                    // nIn, -, info[8] from R + 2
    if ((rc = s.run([&] {
            const int32_t* N = s.dev<int32_t>(oN);
            return pgorb_optimize_sim3_batch_device(c, s.dev<pgorb_keypoint>(oK), N, cap, N + 2, N + 3, 1, s.dev<pgorb_kf_pose>(oPose),
                                                    s.dev<int32_t>(oS), s.dev<int32_t>(oM), new_matches12 ? s.dev<int32_t>(oNM) : nullptr, npoints,
                                                    s.dev<pgorb_map_point>(oP), point_bad ? s.dev(oB) : nullptr, s.dev<pgorb_sim3_estimate>(oE),
                                                    th2, fix_scale, s.dev<pgorb_sim3_estimate>(oEO), s.dev<int32_t>(oMO), s.dev<float>(oC1),
                                                    s.dev<float>(oC2), s.dev<pgorb_kf_pose>(oSP), R + 2, R, nullptr); }))) return rc;
    memcpy(estimate_out, s.host(oEO), sizeof(pgorb_sim3_estimate));
    if (n1) memcpy(matches12_out, s.host(oMO), (size_t)n1 * 4);
    if (chi2_12 && n1) memcpy(chi2_12, s.host(oC1), (size_t)n1 * 4);
    if (chi2_21 && n1) memcpy(chi2_21, s.host(oC2), (size_t)n1 * 4);
    if (scw_pose) memcpy(scw_pose, s.host(oSP), sizeof(pgorb_kf_pose));
    const int32_t* r = s.host<int32_t>(oR);
    if (info) memcpy(info, r + 2, PGORB_OS3_INFO * 4);
    return r[0];
}

}  // extern "C"
