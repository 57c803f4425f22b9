// pose_opt.hip -- Optimizer::PoseOptimization on gfx950: the motion-only refinement of a frame's pose over its map-point slots, one
// workgroup per (frame, pose) problem and one launch per call.
//
// Restates (thirdparty/orb-slam2, thirdparty/g2o):
//   Optimizer::PoseOptimization                   src/Optimizer.cc:239-451 (monocular edges only, mvuRight < 0)
//   Converter::toSE3Quat / toCvMat                src/Converter.cc
//   SE3Quat (exp, operator*, map, normalizeRotation, to_homogeneous_matrix)   g2o/types/se3quat.h
//   EdgeSE3ProjectXYZOnlyPose                     g2o/types/types_six_dof_expmap.{h,cpp} (computeError, linearizeOplus :266-288)
//   BaseUnaryEdge::constructQuadraticForm         g2o/core/base_unary_edge.hpp:43-72, robustInformation base_edge.h:96-102
//   RobustKernelHuber::robustify                  g2o/core/robust_kernel_impl.cpp:78-91
//   OptimizationAlgorithmLevenberg::solve         g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   SparseOptimizer::optimize                     g2o/core/sparse_optimizer.cpp:354-419
//   LinearSolverDense::solve                      g2o/solvers/linear_solver_dense.h:104-112
//   Frame::SetPose / UpdatePoseMatrices           src/Frame.cc
// in double, in the reference's operation order per edge, under the readings of DESIGN.md section 4 (the pose-optimisation rows).  This
// is the project's reading of g2o and Eigen, anchored by the CPU tests of tests/test_pose_optimization.py and not pinned to a g2o build.
// Shared, each in one copy: Huber, the LDLT, Levenberg's step control and the block reductions are g2o_lm.h's (with optimize_sim3.hip,
// local_ba.hip, essential_graph.hip, global_ba.hip); SE3Quat, computeError, toSE3Quat and SetPose are g2o_se3.h's (with local_ba.hip,
// global_ba.hip).  This file's own: EdgeSE3ProjectXYZOnlyPose's Jacobian, which g2o writes with invz and invz2 products where
// EdgeSE3ProjectXYZ divides by z2 (they round differently), and b accumulated as -= (rho1 * J) * w * e where the others add J * r.
//
// k_pose_opt, PO_T threads:
//   1. the slots holding a point are compacted, in keypoint order and by ballot prefix, into edge records (Xw, obs, invSigma2, keypoint,
//      level) in the context's scratch arena;
//   2. edge e belongs to lane e mod PO_T; a lane sums its edges in increasing e into 28 doubles (the 21 upper entries of H, b, chi2),
//      which are reduced by a butterfly inside each wave and then as (w0 + w1) + (w2 + w3) through LDS -- one fixed tree, so a
//      problem's result depends on its inputs alone;
//   3. the Levenberg state (lambda, rho, the LDLT, the estimate) is carried identically by every lane: all waves take the same branches
//      and meet at the same barriers.  Every loop is bounded by 4 rounds x 10 iterations x 10 trials.
#include "match_common.h"
#include "g2o_se3.h"
#include <math.h>
#include <string>

#define PO_T 256
#define PO_WAVES (PO_T / 64)
#define PO_MAX_N 16000            // keypoints per frame, as for the matchers
#define PO_NRED 28                // 21 + 6 + 1

struct PoEdge { float X[3]; float ox, oy, w; int32_t kp; int32_t level; };      // 32 bytes: two 16-byte loads
static_assert(sizeof(PoEdge) == 32, "two dwordx4");

struct PoBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap; const int32_t* pairFrame;
    const pgorb_kf_pose* pose; const int32_t* kpPoint; int npoints; const pgorb_map_point* pts; const uint8_t* pobs;
    int discard, nlevels;
    float invSigma2[PG_MAXL + 1];          // mvInvLevelSigma2 (float, as Frame keeps it)
    PoEdge* edges;                         // [npairs][cap]
    pgorb_kf_pose* poseOut; uint8_t* outlier; int32_t* kpOut; int32_t* nMap; float* chi2; int32_t* info; int32_t* nInl;
};

struct PoCam { double fx, fy, cx, cy; };

// computeError at P of an edge record
__device__ __forceinline__ void po_edge_error(const PoSE3& P, const PoCam& C, const PoEdge& E, double& x, double& y, double& z, double& e0, double& e1)
{
    po_error(P, C.fx, C.fy, C.cx, C.cy, (double)E.X[0], (double)E.X[1], (double)E.X[2], (double)E.ox, (double)E.oy, x, y, z, e0, e1);
}
__device__ __forceinline__ PoEdge po_load_edge(const PoEdge* e)
{
    const float4 a = reinterpret_cast<const float4*>(e)[0], b = reinterpret_cast<const float4*>(e)[1];
    PoEdge E;
    E.X[0] = a.x; E.X[1] = a.y; E.X[2] = a.z; E.ox = a.w; E.oy = b.x; E.w = b.y;
    E.kp = __float_as_int(b.z); E.level = __float_as_int(b.w);
    return E;
}

struct PoShared {
    double part[PO_WAVES][PO_NRED];        // part[0][0 .. 3] also serve the scalar sums
    double red[PO_NRED];
    int cnt[PO_WAVES];
};

// activeRobustChi2 at P over the lane's level-0 edges
__device__ __forceinline__ double po_active_chi2(PoShared& S, const PoEdge* E, int nE, const PoSE3& P, const PoCam& C, bool robust)
{
    double acc = 0.0;
    for (int e = threadIdx.x; e < nE; e += PO_T) {
        const PoEdge ed = po_load_edge(E + e);
        if (ed.level) continue;
        double x, y, z, e0, e1;
        po_edge_error(P, C, ed, x, y, z, e0, e1);
        double c2 = g2o_chi2(e0, e1, (double)ed.w), r0 = c2, r1;
        if (robust) g2o_huber(c2, PO_DELTA, r0, r1);
        acc += r0;
    }
    return g2o_block_sum(S.part[0], acc);
}

__global__ __launch_bounds__(PO_T) void k_pose_opt(PoBatch B)
{
    __shared__ PoShared S;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = B.pairFrame ? B.pairFrame[p] : p;
    const int nf = min(max(B.n[f], 0), B.cap);
    const int64_t row = (int64_t)p * B.cap;
    const pgorb_keypoint* K = B.K + (int64_t)f * B.cap;
    PoEdge* E = B.edges + row;
    const pgorb_kf_pose in = B.pose[p];

    // 1. the edge list, in keypoint order (Optimizer.cc:280-360)
    int nE = 0;
    for (int i0 = 0; i0 < B.cap; i0 += PO_T) {
        const int i = i0 + tid;
        int s = i < nf ? B.kpPoint[row + i] : -1;
        if (s < 0 || s >= B.npoints) s = -1;
        pgorb_keypoint kp;
        if (s >= 0) { kp = K[i]; if (kp.octave < 0 || kp.octave >= B.nlevels) s = -1; }
        const unsigned long long m = __ballot(s >= 0);
        if (lane == 0) S.cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PO_WAVES; w++) { const int c = S.cnt[w]; if (w < wave) before += c; total += c; }
        __syncthreads();
        if (s >= 0) {
            const int e = nE + before + __popcll(m & ((1ull << lane) - 1ull));
            const pgorb_map_point P = B.pts[s];
            float4* dst = reinterpret_cast<float4*>(E + e);
            dst[0] = make_float4(P.pos[0], P.pos[1], P.pos[2], kp.x);
            dst[1] = make_float4(kp.y, B.invSigma2[kp.octave], __int_as_float(i), __int_as_float(0));
        } else if (i < B.cap) {                                         // a slot without a point: its outputs are final
            B.outlier[row + i] = 0;
            if (B.kpOut) B.kpOut[row + i] = -1;
            if (B.chi2) B.chi2[row + i] = 0.0f;
        }
        nE += total;
    }
    __syncthreads();                                                    // a record is written by its keypoint's lane and read by its owner, lane e mod PO_T

    const PoCam C = {(double)in.fx, (double)in.fy, (double)in.cx, (double)in.cy};
    const PoSE3 est0 = po_from_pose(in);                                // Converter::toSE3Quat

    int status = 0, rounds = 0, trials = 0, nBadEdges = 0;
    int its[4] = {0, 0, 0, 0};
    PoSE3 est = est0;
    if (nE < 3) status = PGORB_PO_FEW;                                  // :364
    int nActive = nE;
    for (int it = 0; it < 4 && !status; it++) {
        const bool robust = it <= 2;                                    // setRobustKernel(0) at it == 2 (:407)
        est = est0;                                                     // setEstimate(toSE3Quat(pFrame->mTcw)) (:377)
        PoSE3 errEst = est0;                                            // where the active edges' _error was last computed
        // SparseOptimizer::optimize(10); an empty active set returns at once
        if (nActive > 0) {
            G2oLm lm = {0.0, 2, 0};
            for (int iter = 0; iter < 10; iter++) {
                // computeActiveErrors, activeRobustChi2, buildSystem
                double acc[PO_NRED];
#pragma unroll
                for (int k = 0; k < PO_NRED; k++) acc[k] = 0.0;
                for (int e = tid; e < nE; e += PO_T) {
                    const PoEdge ed = po_load_edge(E + e);
                    if (ed.level) continue;
                    double x, y, z, e0, e1;
                    po_edge_error(est, C, ed, x, y, z, e0, e1);
                    const double w = (double)ed.w;
                    const double c2 = g2o_chi2(e0, e1, w);
                    double rho0 = c2, rho1 = 1.0;
                    if (robust) g2o_huber(c2, PO_DELTA, rho0, rho1);
                    // linearizeOplus (types_six_dof_expmap.cpp:266-288)
                    const double invz = 1.0 / z, invz2 = invz * invz;
                    double J0[6], J1[6];
                    J0[0] = x * y * invz2 * C.fx; J0[1] = -(1.0 + (x * x * invz2)) * C.fx; J0[2] = y * invz * C.fx;
                    J0[3] = -invz * C.fx; J0[4] = 0.0; J0[5] = x * invz2 * C.fx;
                    J1[0] = (1.0 + y * y * invz2) * C.fy; J1[1] = -x * y * invz2 * C.fy; J1[2] = -x * invz * C.fy;
                    J1[3] = 0.0; J1[4] = -invz * C.fy; J1[5] = y * invz2 * C.fy;
                    // constructQuadraticForm: b -= rho1 * A' * omega * e, H += A' * (rho1 * omega) * A (no rho1 factor without the kernel)
                    const double wr = robust ? rho1 * w : w;
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double a0 = J0[i] * wr, a1 = J1[i] * wr;
#pragma unroll
                        for (int j = i; j < 6; j++) acc[k++] += a0 * J0[j] + a1 * J1[j];
                    }
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double a0 = robust ? (rho1 * J0[i]) * w : J0[i] * w, a1 = robust ? (rho1 * J1[i]) * w : J1[i] * w;
                        acc[21 + i] -= a0 * e0 + a1 * e1;
                    }
                    acc[27] += rho0;
                }
                g2o_block_sum_n(S.part, S.red, acc);
                double H[6][6], b[6];
                g2o_dense_system(S.red, H, b);
                double currentChi = S.red[27];
                const double iniChi = currentChi;
                if (!g2o_finite(currentChi)) { status = PGORB_PO_NONFINITE; break; }
                if (iter == 0) g2o_lm_begin(lm, g2o_lm_lambda_init(g2o_max_diagonal(H)));
                its[it]++;
                double rho = 0.0;
                int qmax = 0;
                do {
                    double x[6], scale;
                    const bool ok2 = g2o_dense_trial(H, b, lm.lambda, false, x, scale);
                    const PoSE3 trial = po_oplus(est, x);
                    errEst = trial;
                    const double tempChi = po_active_chi2(S, E, nE, trial, C, robust);
                    if (g2o_lm_decide(lm, currentChi, tempChi, ok2, scale, rho)) est = trial;       // discardTop; else pop
                    qmax++; trials++;
                } while (g2o_lm_again(rho, qmax));
                if (g2o_lm_stop(lm, iniChi, currentChi, qmax, rho)) break;
            }
        }
        if (status) break;
        // the classification (:381-409): an outlier's error is recomputed at the round's result, an inlier keeps the last trial's
        int bad = 0, nonfinite = 0;
        for (int e = tid; e < nE; e += PO_T) {
            PoEdge ed = po_load_edge(E + e);
            double x, y, z, e0, e1;
            po_edge_error(ed.level ? est : errEst, C, ed, x, y, z, e0, e1);
            const double c2 = g2o_chi2(e0, e1, (double)ed.w);
            if (!g2o_finite(c2)) nonfinite = 1;
            const float c2f = __double2float_rn(c2);
            const int out = c2f > 5.991f;
            bad += out;
            E[e].level = out;
            B.outlier[row + ed.kp] = (uint8_t)out;
            if (B.chi2) B.chi2[row + ed.kp] = c2f;
        }
        if (__syncthreads_or(nonfinite)) { status = PGORB_PO_NONFINITE; break; }
        nBadEdges = g2o_block_sum(S.cnt, bad);
        nActive = nE - nBadEdges;
        rounds = it + 1;
        if (nE < 10) break;                                             // optimizer.edges().size() < 10 (:440)
    }

    // the outputs of the slots that hold a point, by the lane that owns the edge, and the count of Tracking.cc:768-787 / :932-950
    const bool untouched = status != 0;
    int kept = 0;
    for (int e = tid; e < nE; e += PO_T) {
        const PoEdge ed = po_load_edge(E + e);
        const int64_t o = row + ed.kp;
        const int s = B.kpPoint[o];
        int out = ed.level;
        if (untouched) { out = 0; if (B.chi2) B.chi2[o] = 0.0f; }
        B.outlier[o] = (uint8_t)((out && !B.discard) ? 1 : 0);
        if (B.kpOut) B.kpOut[o] = (out && B.discard) ? -1 : s;
        kept += (!out && (B.pobs ? B.pobs[s] != 0 : 1)) ? 1 : 0;
    }
    kept = g2o_block_sum(S.cnt, kept);
    if (tid == 0) {
        pgorb_kf_pose o = in;
        if (!untouched) {
            // Converter::toCvMat(SE3Quat), Frame::SetPose, UpdatePoseMatrices: mOw = -mRcw.t() * mtcw
            po_set_pose(est, o);
        }
        B.poseOut[p] = o;
        const int inl = untouched ? 0 : nE - nBadEdges;
        if (B.nInl) B.nInl[p] = inl;
        if (B.nMap) B.nMap[p] = kept;
        if (B.info) {
            int32_t* I = B.info + (int64_t)p * PGORB_PO_INFO;
            I[0] = status; I[1] = rounds; I[2] = its[0]; I[3] = its[1]; I[4] = its[2]; I[5] = its[3]; I[6] = trials; I[7] = nE;
        }
    }
}

// kp_point[i] = source[assigned[i]] where assigned[i] >= 0
__global__ __launch_bounds__(256) void k_slots_from_assignment(const int32_t* __restrict__ assigned, const int32_t* __restrict__ source, int stride,
                                                               int32_t* __restrict__ kpPoint, int cap)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const int a = assigned[(int64_t)p * cap + i];
    if (a >= 0 && a < stride) kpPoint[(int64_t)p * cap + i] = source[(int64_t)p * stride + a];
}

extern "C" {

int pgorb_pose_optimization_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap, const int32_t* d_pair_frame,
        int npairs, const pgorb_kf_pose* d_pose, const int32_t* d_kp_point, int npoints, const pgorb_map_point* d_points,
        const uint8_t* d_point_has_obs, int discard_outliers, pgorb_kf_pose* d_pose_out, uint8_t* d_outlier, int32_t* d_kp_point_out,
        int32_t* d_nmatches_map, float* d_chi2, int32_t* d_info, int32_t* d_ninliers, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || cap < 1 || npairs < 0 || npoints < 0 || (npairs && (!d_pose || !d_kp_point || !d_pose_out || !d_outlier)) ||
        (npoints && !d_points))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_pose_optimization_batch_device");
    if (cap > PO_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pose_optimization: more than 16000 keypoints per frame");
    if (!npairs) return 0;
    PoBatch B;
    B.nlevels = pgorb_levels(c);
    memset(B.invSigma2, 0, sizeof(B.invSigma2));
    if (!(B.nlevels > 0) || B.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, nullptr, B.invSigma2) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    hipStream_t s = (hipStream_t)stream;
    void* scr;
    int rc = pg_ctx_scratch(c, (size_t)npairs * cap * sizeof(PoEdge), s, &scr);
    if (rc) return rc;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.pairFrame = d_pair_frame; B.pose = d_pose; B.kpPoint = d_kp_point; B.npoints = npoints;
    B.pts = d_points; B.pobs = d_point_has_obs; B.discard = discard_outliers ? 1 : 0; B.edges = (PoEdge*)scr;
    B.poseOut = d_pose_out; B.outlier = d_outlier; B.kpOut = d_kp_point_out; B.nMap = d_nmatches_map; B.chi2 = d_chi2; B.info = d_info;
    B.nInl = d_ninliers;
    hipLaunchKernelGGL(k_pose_opt, dim3((unsigned)npairs), dim3(PO_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_pose_opt launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool po_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

int pgorb_pose_optimization(pgorb_ctx* c, const pgorb_keypoint* kps, int n, const pgorb_kf_pose* pose, const int32_t* kp_point, int npoints,
        const pgorb_map_point* points, const uint8_t* point_has_obs, int discard_outliers, pgorb_kf_pose* pose_out, uint8_t* outlier,
        int32_t* kp_point_out, int32_t* nmatches_map, float* chi2, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    if (n < 0 || npoints < 0) why = "a count is negative";
    else if (!pose || !pose_out || (n && (!kps || !kp_point || !outlier)) || (npoints && !points)) why = "an array that is read is NULL";
    else if (!po_all_finite(pose->Tcw, 12) || !po_all_finite(&pose->fx, 4)) why = "the pose or the camera is not finite";
    else if (pose->fx == 0.0f || pose->fy == 0.0f) why = "fx or fy is zero";
    for (int i = 0; !why && i < n; i++) {
        const int s = kp_point[i];
        if (s < -1 || s >= npoints) why = "a slot's point index is out of range";
        else if (s >= 0 && (kps[i].octave < 0 || kps[i].octave >= nlevels)) why = "an octave is outside the context's levels";
        else if (s >= 0 && !po_all_finite(points[s].pos, 3)) why = "a referenced point is not finite";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_pose_optimization: ") + why).c_str());
    if (n > PO_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pose_optimization: more than 16000 keypoints per frame");
    const int cap = std::max(n, 1), np = std::max(npoints, 1);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)cap * sizeof(pgorb_keypoint)), oPose = s.region(PG_UP, sizeof(pgorb_kf_pose)),
                 oKP = s.region(PG_UP, (size_t)cap * 4), oP = s.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)),
                 oO = s.region(PG_UP, point_has_obs ? np : 0), oPO = s.region(PG_DOWN, sizeof(pgorb_kf_pose)), oOut = s.region(PG_DOWN, cap),
                 oKO = s.region(PG_DOWN, (size_t)cap * 4), oChi = s.region(PG_DOWN, (size_t)cap * 4), oR = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t cnt[4] = {n, 0, 0, 0};
    s.put(oN, cnt, 16);
    s.put(oK, kps, (size_t)n * sizeof(pgorb_keypoint), 0, (size_t)cap * sizeof(pgorb_keypoint));
    s.put(oPose, pose, sizeof(pgorb_kf_pose));
    memset(s.host(oKP), 0xFF, (size_t)cap * 4);
    s.put(oKP, kp_point, (size_t)n * 4);
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    if (point_has_obs) s.put(oO, point_has_obs, npoints, 0, np);
    int32_t* R = s.dev<int32_t>(oR);                                    // nmatches_map, ninliers, info[8]
    if ((rc = s.run([&] {
            return pgorb_pose_optimization_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), cap, nullptr, 1, s.dev<pgorb_kf_pose>(oPose),
                                                        s.dev<int32_t>(oKP), npoints, s.dev<pgorb_map_point>(oP), point_has_obs ? s.dev(oO) : nullptr,
                                                        discard_outliers, s.dev<pgorb_kf_pose>(oPO), s.dev(oOut), s.dev<int32_t>(oKO), R,
                                                        s.dev<float>(oChi), R + 2, R + 1, nullptr); }))) return rc;
    memcpy(pose_out, s.host(oPO), sizeof(pgorb_kf_pose));
    if (n) memcpy(outlier, s.host(oOut), n);
    if (kp_point_out) memcpy(kp_point_out, s.host(oKO), (size_t)n * 4);
    if (chi2) memcpy(chi2, s.host(oChi), (size_t)n * 4);
    const int32_t* r = s.host<int32_t>(oR);
    if (nmatches_map) *nmatches_map = r[0];
    if (info) memcpy(info, r + 2, PGORB_PO_INFO * 4);
    return r[1];
}

int pgorb_slots_from_assignment_batch_device(pgorb_ctx* c, const int32_t* d_assigned, const int32_t* d_source, int source_stride,
        int32_t* d_kp_point, int cap_per_frame, int npairs, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (cap_per_frame < 1 || npairs < 0 || source_stride < 0 || (npairs && (!d_assigned || !d_kp_point || (source_stride && !d_source))))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_slots_from_assignment_batch_device");
    if (!npairs) return 0;
    hipLaunchKernelGGL(k_slots_from_assignment, dim3((unsigned)((cap_per_frame + 255) / 256), (unsigned)npairs), dim3(256), 0, (hipStream_t)stream,
                       d_assigned, d_source, source_stride, d_kp_point, cap_per_frame);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_slots_from_assignment launch failed");
    return 0;
}

// the same over host arrays: no device is involved
int pgorb_slots_from_assignment(pgorb_ctx* c, const int32_t* assigned, const int32_t* source, int nsource, int32_t* kp_point, int n)
{
    if (!c) return PGORB_E_ARG;
    if (n < 0 || nsource < 0 || (n && (!assigned || !kp_point)) || (nsource && !source))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_slots_from_assignment: a count is negative or a pointer is NULL");
    for (int i = 0; i < n; i++)
        if (assigned[i] < -1 || assigned[i] >= nsource) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_slots_from_assignment: an assignment is out of range");
    for (int i = 0; i < n; i++)
        if (assigned[i] >= 0) kp_point[i] = source[assigned[i]];
    return 0;
}

}  // extern "C"
