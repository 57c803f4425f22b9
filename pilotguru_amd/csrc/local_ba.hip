// local_ba.hip -- Optimizer::LocalBundleAdjustment on gfx950: the bundle adjustment of a window of key frames and the map points
// they hold, one workgroup per window.
//
// Restates (thirdparty/orb-slam2, thirdparty/g2o):
//   Optimizer::LocalBundleAdjustment              src/Optimizer.cc:453-778 (monocular edges only, mvuRight < 0)
//   Converter::toSE3Quat / toCvMat                src/Converter.cc
//   VertexSE3Expmap / VertexSBAPointXYZ (oplus)   g2o/types/types_six_dof_expmap.h, types_sba.h
//   EdgeSE3ProjectXYZ                             g2o/types/types_six_dof_expmap.{h,cpp} (computeError, isDepthPositive, linearizeOplus :103-139)
//   BaseBinaryEdge::constructQuadraticForm        g2o/core/base_binary_edge.hpp:60-116
//   RobustKernelHuber::robustify                  g2o/core/robust_kernel_impl.cpp:78-91
//   BlockSolver_6_3 (buildSystem, setLambda, solve)   g2o/core/block_solver.hpp:353-589
//   OptimizationAlgorithmLevenberg::solve         g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   SparseOptimizer::optimize / initializeOptimization   g2o/core/sparse_optimizer.cpp
//   KeyFrame::SetPose                             src/KeyFrame.cc
// in double, under the ten readings of DESIGN.md section 5 (the local-bundle-adjustment rows of section 4).  This is the project's
// reading of g2o and Eigen, anchored by the CPU tests of tests/test_local_bundle_adjustment.py and not pinned to a g2o build.
// Shared, each in one copy: Huber, Levenberg's step control, the block reductions and the 3 x 3 inverse are g2o_lm.h's (with
// pose_opt.hip, optimize_sim3.hip, essential_graph.hip, global_ba.hip); SE3Quat, EdgeSE3ProjectXYZ's error and linearisation,
// toSE3Quat and SetPose are g2o_se3.h's (the linearisation with global_ba.hip, the rest with pose_opt.hip as well).
//
// k_lba_prepare, one workgroup per window: the flags (role per frame, is_local per point), the window's point list in table order
// with each point's CSR range, its cameras in frame order, the integer half of every edge record, and each free camera's edge list.
// k_lba, one workgroup of LBA_T threads per window, Levenberg's control flow inside the kernel.  Who sums what, in which order:
//   * a POINT belongs to thread j mod LBA_T (j = its place in the window's list).  That thread linearises the point's edges in CSR
//     order, sums Hll and bl in that order, inverts Hll + lambda, back-substitutes and moves the point;
//   * a ROW of the reduced camera system belongs to thread row mod LBA_T.  That thread walks its camera's edges (a list k_lba_prepare
//     builds once: the window's points in list order, a point's edges in CSR order) and sums its row of Hpp and bp (once per
//     iteration) and of Hschur = Hpp - sum Bi Dinv Bj' and bschur (once per trial) in that order;
//   * chi2 and computeScale: every thread sums its own items in order; a xor butterfly inside each wave, then (w0 + w1) + (w2 + w3);
//   * the reduced system lives in the scratch arena; the Cholesky R'R runs over its upper triangle in index order, one barrier pair a
//     column, and each entry is updated by one thread in increasing k.
// No atomics; a window's result depends on its inputs alone.  Every loop is bounded: 2 rounds x 10 iterations x 10 trials.
// The per-edge records are addressed by CSR position and the per-point records by table index: the windows of one call hold disjoint
// local points (the header states the rule), so they never meet there, and a caller who breaks the rule stays inside the arrays.
#include "match_common.h"
#include "g2o_se3.h"
#include <math.h>
#include <string>
#include <vector>

#define LBA_T 256
#define LBA_WAVES (LBA_T / 64)
#define LBA_MAX_N 16000           // keypoints per frame, as for the matchers
#define LBA_ROLE_LISTED_BAD 3     // a bad key frame named by the window (mnBALocalForKF is set for it, :465): never fixed; reported as none

// the double half of an edge record
enum { LE_ERR = 0, LE_WO = 2, LE_R = 3, LE_JJ = 5, LE_W = 17, LBA_EDGE_D = 36 };
// a point record
enum { LP_X = 0, LP_XT = 3, LP_HLL = 6, LP_BL = 15, LP_DINV = 18, LP_DB = 27, LBA_PT_D = 30 };

struct LbaEdgeI { int32_t cam, col, level; float ox, oy, w; int32_t pad0, pad1; };       // cam < 0: the observation is no edge
static_assert(sizeof(LbaEdgeI) == 32, "two dwordx4");
struct LbaCam { PoSE3 est, trial; double fx, fy, cx, cy; int32_t frame, col, active, role; };
struct LbaHdr { int32_t status, nE, nPts, nCam, nLocal, nFixed, nFree, pad; };

struct LbaBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap, nframes;
    const pgorb_kf_pose* pose; const uint8_t* kfBad; const int32_t* kfPoint; const uint8_t* id0;
    const int32_t* winStart; const int32_t* winKf; int nwin, nwinKf;
    int npoints; pgorb_map_point* pts; const uint8_t* ptBad; const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs;
    int rounds, nlevels;
    float invSigma2[PG_MAXL + 1];          // mvInvLevelSigma2 (float, as KeyFrame keeps it)
    pgorb_kf_pose* poseOut; uint8_t* erase; float* chi2; uint8_t* level; uint8_t* isLocal; uint8_t* role; int32_t* info; int32_t* nErased;
    // the scratch arena: shared records, then one block per window
    LbaEdgeI* eI; double* eD; double* pD; int32_t* pAct;
    uint8_t* win; size_t winBytes, oPtList, oRange, oCam, oHpp, oHs, oFrameCam, oCamStart, oCamEdge;
    int capP, capC, capL, capE;
};

struct LbaShared {
    double part[LBA_WAVES];
    int cnt[LBA_WAVES], cnt2[LBA_WAVES];
    int freeCam[PGORB_LBA_MAX_LOCAL_KF];
    double bp[6 * PGORB_LBA_MAX_LOCAL_KF], x[6 * PGORB_LBA_MAX_LOCAL_KF];
};

// the place of a flagged thread among the block's flagged threads, in thread order; total = how many there are
__device__ __forceinline__ int lba_rank(int* cnt, bool in, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(in);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < LBA_WAVES; w++) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
    __syncthreads();
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

struct LbaWin {
    LbaHdr* H; int32_t* ptList; int2* range; LbaCam* cams; double* Hpp; double* Hs; int32_t* frameCam;
    int32_t* camStart; int2* camEdge;       // the edges of free camera c in walk order: (CSR position, place of the point in ptList)
};
__device__ __forceinline__ LbaWin lba_window(const LbaBatch& B, int w)
{
    uint8_t* blk = B.win + (size_t)w * B.winBytes;
    LbaWin W;
    W.H = (LbaHdr*)blk; W.ptList = (int32_t*)(blk + B.oPtList); W.range = (int2*)(blk + B.oRange); W.cams = (LbaCam*)(blk + B.oCam);
    W.Hpp = (double*)(blk + B.oHpp); W.Hs = (double*)(blk + B.oHs); W.frameCam = (int32_t*)(blk + B.oFrameCam);
    W.camStart = (int32_t*)(blk + B.oCamStart); W.camEdge = (int2*)(blk + B.oCamEdge);
    return W;
}

// ---- the sets of Optimizer.cc:455-504 as flags, and the lists the solver walks
__global__ __launch_bounds__(LBA_T) void k_lba_prepare(LbaBatch B)
{
    __shared__ LbaShared S;
    const int w = blockIdx.x, tid = threadIdx.x;
    const LbaWin W = lba_window(B, w);
    uint8_t* role = B.role + (size_t)w * B.nframes;
    uint8_t* isLocal = B.isLocal + (size_t)w * B.npoints;
    int ws = max(B.winStart[w], 0), we = min(B.winStart[w + 1], B.nwinKf);
    if (we < ws) we = ws;
    for (int f = tid; f < B.nframes; f += LBA_T) { role[f] = 0; W.frameCam[f] = -1; }
    for (int p = tid; p < B.npoints; p += LBA_T) isLocal[p] = 0;
    __syncthreads();
    // lLocalKeyFrames (:456-468); a key frame named twice gets the same byte twice
    for (int i = ws + tid; i < we; i += LBA_T) {
        const int f = B.winKf[i];
        if (f >= 0 && f < B.nframes) role[f] = (B.kfBad && B.kfBad[f]) ? LBA_ROLE_LISTED_BAD : PGORB_LBA_ROLE_LOCAL;
    }
    __syncthreads();
    // lLocalMapPoints (:470-486): the live points in the slots of the local key frames
    for (int i = ws; i < we; i++) {
        const int f = B.winKf[i];
        if (f < 0 || f >= B.nframes || role[f] != PGORB_LBA_ROLE_LOCAL) continue;
        const int nf = min(max(B.n[f], 0), B.cap);
        for (int s = tid; s < nf; s += LBA_T) {
            const int p = B.kfPoint[(int64_t)f * B.cap + s];
            if (p >= 0 && p < B.npoints && !(B.ptBad && B.ptBad[p])) isLocal[p] = 1;
        }
    }
    __syncthreads();
    int nPts = 0;
    for (int p0 = 0; p0 < B.npoints; p0 += LBA_T) {
        const int p = p0 + tid;
        const bool in = p < B.npoints && isLocal[p];
        int total;
        const int j = nPts + lba_rank(S.cnt, in, total);
        if (in && j < B.capP) {
            W.ptList[j] = p;
            int a = B.obsStart[p], b = B.obsStart[p + 1];
            if (a < 0 || b > B.nobs || b < a) a = b = 0;              // a list outside the arrays is an empty list
            W.range[j] = make_int2(a, b);
        }
        nPts += total;
    }
    __syncthreads();
    const int nP = min(nPts, B.capP);
    // the edges (:585-589) and lFixedCameras (:488-504): every observation of a local point in a frame that is not bad
    int cnt = 0;
    for (int j = tid; j < nP; j += LBA_T) {
        const int2 r = W.range[j];
        for (int k = r.x; k < r.y; k++) {
            const int f = B.obsFrame[k], i = B.obsIdx[k];
            bool ok = f >= 0 && f < B.nframes && !(B.kfBad && B.kfBad[f]);
            if (ok) ok = i >= 0 && i < min(max(B.n[f], 0), B.cap);
            if (ok) { const int o = B.K[(int64_t)f * B.cap + i].octave; ok = o >= 0 && o < B.nlevels; }
            if (ok) { if (role[f] == 0) role[f] = PGORB_LBA_ROLE_FIXED; cnt++; }
            B.eI[k].cam = ok ? -2 : -1;
        }
    }
    const int nE = g2o_block_sum(S.cnt, cnt);                               // (its barriers also publish the roles)
    // the cameras in frame order; the free ones (local and not the key frame with mnId 0, :529) get the columns of the reduced system
    int nCam = 0, nFree = 0, nLocal = 0;
    for (int f0 = 0; f0 < B.nframes; f0 += LBA_T) {
        const int f = f0 + tid;
        const int ro = f < B.nframes ? role[f] : 0;
        const bool in = ro == PGORB_LBA_ROLE_LOCAL || ro == PGORB_LBA_ROLE_FIXED;
        const bool fr = ro == PGORB_LBA_ROLE_LOCAL && !(B.id0 && B.id0[f]);
        int total, totalFree, totalLocal;
        const int c = nCam + lba_rank(S.cnt, in, total);
        const int col = nFree + lba_rank(S.cnt2, fr, totalFree);
        lba_rank(S.cnt, ro == PGORB_LBA_ROLE_LOCAL, totalLocal);
        if (in && c < B.capC) {
            LbaCam& C = W.cams[c];
            C.frame = f; C.role = ro; C.col = (fr && col < B.capL) ? col : -1; C.active = 0;
            W.frameCam[f] = c;
        }
        if (ro == LBA_ROLE_LISTED_BAD) role[f] = 0;
        nCam += total; nFree += totalFree; nLocal += totalLocal;
    }
    __syncthreads();
    for (int j = tid; j < nP; j += LBA_T) {
        const int2 r = W.range[j];
        for (int k = r.x; k < r.y; k++) {
            if (B.eI[k].cam != -2) continue;
            const int f = B.obsFrame[k], c = W.frameCam[f];
            LbaEdgeI e;
            e.cam = -1; e.col = -1; e.level = 0; e.ox = e.oy = e.w = 0.0f; e.pad0 = e.pad1 = 0;
            if (c >= 0) {
                const pgorb_keypoint kp = B.K[(int64_t)f * B.cap + B.obsIdx[k]];
                e.cam = c; e.col = W.cams[c].col; e.ox = kp.x; e.oy = kp.y; e.w = B.invSigma2[kp.octave];
            }
            B.eI[k] = e;
        }
    }
    __syncthreads();
    // the edges of each free camera in the order the row walks take them (points in list order, a point's edges in CSR order): count,
    // prefix, fill -- once per call, so the walks of k_lba touch a camera's own edges and not every record of the window
    const int nF = min(nFree, B.capL);
    for (int c = tid; c < nF; c += LBA_T) {
        int n = 0;
        for (int j = 0; j < nP; j++) {
            const int2 r = W.range[j];
            for (int k = r.x; k < r.y; k++) n += (B.eI[k].cam >= 0 && B.eI[k].col == c) ? 1 : 0;
        }
        W.camStart[c + 1] = n;
    }
    __syncthreads();
    if (tid == 0) {
        W.camStart[0] = 0;
        for (int c = 0; c < nF; c++) W.camStart[c + 1] += W.camStart[c];
    }
    __syncthreads();
    for (int c = tid; c < nF; c += LBA_T) {
        int at = W.camStart[c];
        for (int j = 0; j < nP; j++) {
            const int2 r = W.range[j];
            for (int k = r.x; k < r.y; k++)
                if (B.eI[k].cam >= 0 && B.eI[k].col == c) { if (at < B.capE) W.camEdge[at] = make_int2(k, j); at++; }
        }
    }
    if (tid == 0) {
        LbaHdr h;
        h.nE = nE; h.nPts = nPts; h.nCam = nCam; h.nLocal = nLocal; h.nFixed = nCam - nLocal; h.nFree = nFree; h.pad = 0;
        h.status = 0;
        if (nPts > PGORB_LBA_MAX_POINTS || nLocal > PGORB_LBA_MAX_LOCAL_KF || h.nFixed > PGORB_LBA_MAX_FIXED_KF || nE > PGORB_LBA_MAX_EDGES)
            h.status = PGORB_LBA_LIMIT;
        else if (nE == 0) h.status = PGORB_LBA_NOTHING;
        *W.H = h;
    }
}

// activeRobustChi2 at the trial estimates (computeActiveErrors stores every active edge's _error: reading 6)
__device__ __forceinline__ double lba_trial_chi2(LbaShared& S, const LbaBatch& B, const LbaWin& W, int nP, bool robust)
{
    double acc = 0.0;
    for (int j = threadIdx.x; j < nP; j += LBA_T) {
        const int p = W.ptList[j];
        if (!B.pAct[p]) continue;
        const double* PD = B.pD + (int64_t)p * LBA_PT_D;
        const int2 r = W.range[j];
        double chiP = 0.0;
        for (int k = r.x; k < r.y; k++) {
            const LbaEdgeI e = B.eI[k];
            if (e.cam < 0 || e.level) continue;
            const LbaCam& C = W.cams[e.cam];
            double x, y, z, e0, e1;
            po_error(C.trial, C.fx, C.fy, C.cx, C.cy, PD[LP_XT], PD[LP_XT + 1], PD[LP_XT + 2], (double)e.ox, (double)e.oy, x, y, z, e0, e1);
            double* ED = B.eD + (int64_t)k * LBA_EDGE_D;
            ED[LE_ERR] = e0; ED[LE_ERR + 1] = e1;
            double c2 = g2o_chi2(e0, e1, (double)e.w), r0 = c2, r1;
            if (robust) g2o_huber(c2, PO_DELTA, r0, r1);
            chiP += r0;
        }
        acc += chiP;
    }
    return g2o_block_sum(S.part, acc);
}

// e->chi2() > 5.991 || !e->isDepthPositive() over every edge: chi2 of the stored _error, the depth at the estimates (readings 6, 7).
// final = false: setLevel(1) (:680-683); final = true: vToErase and the per-observation outputs (:715-728).  Returns how many; -1 = a chi2 is not finite.
__device__ __forceinline__ int lba_classify(LbaShared& S, const LbaBatch& B, const LbaWin& W, int nP, int w, bool final)
{
    int bad = 0, nonfinite = 0;
    for (int j = threadIdx.x; j < nP; j += LBA_T) {
        const int p = W.ptList[j];
        const double* PD = B.pD + (int64_t)p * LBA_PT_D;
        const int2 r = W.range[j];
        for (int k = r.x; k < r.y; k++) {
            const LbaEdgeI e = B.eI[k];
            if (e.cam < 0) continue;
            const double* ED = B.eD + (int64_t)k * LBA_EDGE_D;
            const double c2 = g2o_chi2(ED[LE_ERR], ED[LE_ERR + 1], (double)e.w);
            if (!g2o_finite(c2)) nonfinite = 1;
            const LbaCam& C = W.cams[e.cam];
            double rx, ry, rz;
            g2o_rotate(C.est, PD[LP_X], PD[LP_X + 1], PD[LP_X + 2], rx, ry, rz);
            const int out = (c2 > 5.991 || !(rz + C.est.tz > 0.0)) ? 1 : 0;
            bad += out;
            if (!final) B.eI[k].level = out;
            else if (B.erase) {
                const int64_t o = (int64_t)w * B.nobs + k;
                B.erase[o] = (uint8_t)out; B.chi2[o] = __double2float_rn(c2); B.level[o] = (uint8_t)e.level;
            }
        }
    }
    if (__syncthreads_or(nonfinite)) return -1;
    return g2o_block_sum(S.cnt, bad);
}

__global__ __launch_bounds__(LBA_T) void k_lba(LbaBatch B)
{
    __shared__ LbaShared S;
    const int w = blockIdx.x, tid = threadIdx.x;
    const LbaWin W = lba_window(B, w);
    const LbaHdr H = *W.H;
    const int nP = min(H.nPts, B.capP), nCam = min(H.nCam, B.capC), nFree = min(H.nFree, B.capL), n6 = 6 * nFree;
    int status = H.status;

    // the vertices: Converter::toSE3Quat of each camera's float Tcw, Converter::toVector3d of each local point
    for (int c = tid; c < nCam; c += LBA_T) {
        LbaCam& C = W.cams[c];
        const pgorb_kf_pose in = B.pose[C.frame];
        const PoSE3 E = po_from_pose(in);
        C.est = E; C.trial = E;
        C.fx = (double)in.fx; C.fy = (double)in.fy; C.cx = (double)in.cx; C.cy = (double)in.cy;
        if (C.col >= 0) S.freeCam[C.col] = c;
    }
    for (int j = tid; j < nP; j += LBA_T) {
        const int p = W.ptList[j];
        double* PD = B.pD + (int64_t)p * LBA_PT_D;
        const pgorb_map_point P = B.pts[p];
#pragma unroll
        for (int m = 0; m < 3; m++) { PD[LP_X + m] = (double)P.pos[m]; PD[LP_XT + m] = (double)P.pos[m]; }
    }
    __syncthreads();

    int its[2] = {0, 0}, trials[2] = {0, 0}, nLevel1 = 0, nErase = 0;
    for (int round = 0; round < B.rounds && !status; round++) {
        const bool robust = round == 0;                                 // setRobustKernel(0) before the second optimize (:685)
        const int iterations = round == 0 ? 5 : 10;
        // initializeOptimization(0): a vertex without a level-0 edge takes no part (reading 8)
        for (int c = tid; c < nCam; c += LBA_T) W.cams[c].active = 0;
        __syncthreads();
        int nAct = 0;
        for (int j = tid; j < nP; j += LBA_T) {
            const int2 r = W.range[j];
            int a = 0;
            for (int k = r.x; k < r.y; k++) {
                const LbaEdgeI e = B.eI[k];
                if (e.cam < 0 || e.level) continue;
                a++;
                W.cams[e.cam].active = 1;                               // the same word from every thread that writes it
            }
            B.pAct[W.ptList[j]] = a > 0;
            nAct += a;
        }
        nAct = g2o_block_sum(S.cnt, nAct);
        if (nAct == 0) continue;                                        // optimize() over an empty active set returns at once

        G2oLm lm = {0.0, 2, 0};
        for (int iter = 0; iter < iterations && !status; iter++) {
            // computeActiveErrors, activeRobustChi2, buildSystem: the landmark half, point by point
            double acc = 0.0, maxd = 0.0;
            for (int j = tid; j < nP; j += LBA_T) {
                const int p = W.ptList[j];
                if (!B.pAct[p]) continue;
                double* PD = B.pD + (int64_t)p * LBA_PT_D;
                const int2 r = W.range[j];
                double Hl[9], bl[3], chiP = 0.0;
#pragma unroll
                for (int m = 0; m < 9; m++) Hl[m] = 0.0;
                bl[0] = bl[1] = bl[2] = 0.0;
                for (int k = r.x; k < r.y; k++) {
                    const LbaEdgeI e = B.eI[k];
                    if (e.cam < 0 || e.level) continue;
                    const LbaCam& C = W.cams[e.cam];
                    const PoSE3 P = C.est;
                    PoLin L;
                    double Ji0[3], Ji1[3];
                    po_linearize_xyz(P, C.fx, C.fy, C.cx, C.cy, PD + LP_X, (double)e.ox, (double)e.oy, (double)e.w, robust, PO_DELTA, L);
                    po_point_jacobian(P, C.fx, C.fy, L, Ji0, Ji1);
                    chiP += L.rho0;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int b = 0; b < 3; b++) Hl[a * 3 + b] += (Ji0[a] * L.wO) * Ji0[b] + (Ji1[a] * L.wO) * Ji1[b];
                        bl[a] += Ji0[a] * L.r0 + Ji1[a] * L.r1;
                    }
                    double* ED = B.eD + (int64_t)k * LBA_EDGE_D;
                    ED[LE_ERR] = L.e0; ED[LE_ERR + 1] = L.e1; ED[LE_WO] = L.wO; ED[LE_R] = L.r0; ED[LE_R + 1] = L.r1;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        ED[LE_JJ + a] = L.Jj0[a]; ED[LE_JJ + 6 + a] = L.Jj1[a];
#pragma unroll
                        for (int m = 0; m < 3; m++) ED[LE_W + a * 3 + m] = (L.Jj0[a] * L.wO) * Ji0[m] + (L.Jj1[a] * L.wO) * Ji1[m];
                    }
                }
#pragma unroll
                for (int m = 0; m < 9; m++) PD[LP_HLL + m] = Hl[m];
#pragma unroll
                for (int m = 0; m < 3; m++) PD[LP_BL + m] = bl[m];
                maxd = fmax(fmax(fabs(Hl[0]), fabs(Hl[4])), fmax(fabs(Hl[8]), maxd));
                acc += chiP;
            }
            double currentChi = g2o_block_sum(S.part, acc);
            const double iniChi = currentChi;
            if (!g2o_finite(currentChi)) { status = PGORB_LBA_NONFINITE; break; }
            // the camera half: each row of Hpp and bp by its own thread, over the points in list order
            for (int row = tid; row < n6; row += LBA_T) {
                const int c = row / 6, r = row % 6;
                double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b = 0.0;
                if (W.cams[S.freeCam[c]].active)
                    for (int e = W.camStart[c], e1 = min(W.camStart[c + 1], B.capE); e < e1; e++) {
                        const int k = W.camEdge[e].x;
                        if (B.eI[k].level) continue;
                        const double* ED = B.eD + (int64_t)k * LBA_EDGE_D;
                        const double a0 = ED[LE_JJ + r] * ED[LE_WO], a1 = ED[LE_JJ + 6 + r] * ED[LE_WO];
#pragma unroll
                        for (int cc = 0; cc < 6; cc++) h[cc] += a0 * ED[LE_JJ + cc] + a1 * ED[LE_JJ + 6 + cc];
                        b += ED[LE_JJ + r] * ED[LE_R] + ED[LE_JJ + 6 + r] * ED[LE_R + 1];
                    }
#pragma unroll
                for (int cc = 0; cc < 6; cc++) W.Hpp[row * 6 + cc] = h[cc];
                S.bp[row] = b;
                maxd = fmax(fabs(h[r]), maxd);
            }
            if (iter == 0) {                                            // computeLambdaInit over every active vertex (reading 5); the barriers publish Hpp, bp
                g2o_lm_begin(lm, g2o_lm_lambda_init(g2o_block_max(S.part, maxd)));
            } else __syncthreads();
            its[round]++;
            double rho = 0.0;
            int qmax = 0;
            do {
                const double lambda = lm.lambda;
                // setLambda on both diagonals; Dinv = D->inverse(), db = Dinv * bl (block_solver.hpp:385-395)
                for (int j = tid; j < nP; j += LBA_T) {
                    const int p = W.ptList[j];
                    if (!B.pAct[p]) continue;
                    double* PD = B.pD + (int64_t)p * LBA_PT_D;
                    double D[9], I[9];
#pragma unroll
                    for (int m = 0; m < 9; m++) D[m] = PD[LP_HLL + m];
                    D[0] += lambda; D[4] += lambda; D[8] += lambda;
                    g2o_inverse3(D, I);
#pragma unroll
                    for (int m = 0; m < 9; m++) PD[LP_DINV + m] = I[m];
#pragma unroll
                    for (int m = 0; m < 3; m++) PD[LP_DB + m] = (I[m * 3] * PD[LP_BL] + I[m * 3 + 1] * PD[LP_BL + 1]) + I[m * 3 + 2] * PD[LP_BL + 2];
                }
                __syncthreads();
                // Hschur = Hpp - sum Bi Dinv Bj' over the upper block triangle, bschur = bp - sum Bi Dinv bl (:381-439): a row a thread.
                // A camera without a level-0 edge keeps a unit diagonal and a zero right side: it decouples and its update is 0.
                for (int row = tid; row < n6; row += LBA_T) {
                    const int c = row / 6, r = row % 6;
                    double* Hrow = W.Hs + (int64_t)row * n6;
                    const bool act = W.cams[S.freeCam[c]].active != 0;
                    for (int col = c * 6; col < n6; col++) Hrow[col] = 0.0;
#pragma unroll
                    for (int cc = 0; cc < 6; cc++) Hrow[c * 6 + cc] = act ? (cc == r ? W.Hpp[row * 6 + cc] + lambda : W.Hpp[row * 6 + cc]) : (cc == r ? 1.0 : 0.0);
                    double coef = 0.0;
                    if (act)
                        for (int e = W.camStart[c], e1 = min(W.camStart[c + 1], B.capE); e < e1; e++) {
                            const int2 kj = W.camEdge[e];
                            const int ka = kj.x, j = kj.y;
                            if (B.eI[ka].level) continue;
                            const int2 rg = W.range[j];
                            const double* PD = B.pD + (int64_t)W.ptList[j] * LBA_PT_D;
                            const double* Wa = B.eD + (int64_t)ka * LBA_EDGE_D + LE_W + r * 3;
                            double v[3];
#pragma unroll
                            for (int m = 0; m < 3; m++) v[m] = (Wa[0] * PD[LP_DINV + m] + Wa[1] * PD[LP_DINV + 3 + m]) + Wa[2] * PD[LP_DINV + 6 + m];
                            coef += (Wa[0] * PD[LP_DB] + Wa[1] * PD[LP_DB + 1]) + Wa[2] * PD[LP_DB + 2];
                            for (int k = rg.x; k < rg.y; k++) {
                                const int cb = B.eI[k].col;
                                if (cb < c || B.eI[k].cam < 0 || B.eI[k].level) continue;
                                const double* Wb = B.eD + (int64_t)k * LBA_EDGE_D + LE_W;
#pragma unroll
                                for (int cc = 0; cc < 6; cc++) Hrow[cb * 6 + cc] -= (v[0] * Wb[cc * 3] + v[1] * Wb[cc * 3 + 1]) + v[2] * Wb[cc * 3 + 2];
                            }
                        }
                    S.x[row] = act ? S.bp[row] - coef : 0.0;
                }
                __syncthreads();
                // LinearSolverEigen read as a dense Cholesky R'R of the upper triangle in index order; a pivot that is not positive fails
                bool ok2 = true;
                for (int k = 0; k < n6; k++) {
                    const double d = W.Hs[(int64_t)k * n6 + k];
                    if (!(d > 0.0)) { ok2 = false; break; }
                    const double rk = __dsqrt_rn(d);
                    __syncthreads();                                    // everyone has read the pivot
                    if (tid == 0) W.Hs[(int64_t)k * n6 + k] = rk;
                    for (int j = k + 1 + tid; j < n6; j += LBA_T) W.Hs[(int64_t)k * n6 + j] /= rk;
                    __syncthreads();
                    for (int i = k + 1 + (tid >> 6); i < n6; i += LBA_WAVES) {           // a wave a row, its lanes over the columns j >= i
                        const double rki = W.Hs[(int64_t)k * n6 + i];
                        for (int j = i + (tid & 63); j < n6; j += 64) W.Hs[(int64_t)i * n6 + j] -= rki * W.Hs[(int64_t)k * n6 + j];
                    }
                    __syncthreads();
                }
                __syncthreads();
                if (ok2) {
                    for (int k = 0; k < n6; k++) {                      // R' y = bschur
                        if (tid == 0) S.x[k] = S.x[k] / W.Hs[(int64_t)k * n6 + k];
                        __syncthreads();
                        const double yk = S.x[k];
                        for (int j = k + 1 + tid; j < n6; j += LBA_T) S.x[j] -= W.Hs[(int64_t)k * n6 + j] * yk;
                        __syncthreads();
                    }
                    for (int k = n6 - 1; k >= 0; k--) {                 // R x = y
                        if (tid == 0) S.x[k] = S.x[k] / W.Hs[(int64_t)k * n6 + k];
                        __syncthreads();
                        const double xk = S.x[k];
                        for (int i = tid; i < k; i += LBA_T) S.x[i] -= W.Hs[(int64_t)i * n6 + k] * xk;
                        __syncthreads();
                    }
                } else {
                    for (int row = tid; row < n6; row += LBA_T) S.x[row] = 0.0;      // a failed factorisation: the trial stays at the estimates
                    __syncthreads();
                }
                // xl = Dinv * (bl - B' xp) (:459-483), update(), and computeScale's terms: the camera rows first, then the points
                double sc = 0.0;
                for (int row = tid; row < n6; row += LBA_T) sc += S.x[row] * (lambda * S.x[row] + S.bp[row]);
                for (int c = tid; c < nFree; c += LBA_T) {
                    LbaCam& C = W.cams[S.freeCam[c]];
                    if (ok2 && C.active) {
                        const double u[6] = {S.x[c * 6], S.x[c * 6 + 1], S.x[c * 6 + 2], S.x[c * 6 + 3], S.x[c * 6 + 4], S.x[c * 6 + 5]};
                        C.trial = po_oplus(C.est, u);
                    } else C.trial = C.est;
                }
                for (int j = tid; j < nP; j += LBA_T) {
                    const int p = W.ptList[j];
                    if (!B.pAct[p]) continue;
                    double* PD = B.pD + (int64_t)p * LBA_PT_D;
                    double xl[3] = {0.0, 0.0, 0.0};
                    if (ok2) {
                        double cl[3] = {PD[LP_BL], PD[LP_BL + 1], PD[LP_BL + 2]};
                        const int2 rg = W.range[j];
                        for (int k = rg.x; k < rg.y; k++) {
                            const LbaEdgeI e = B.eI[k];
                            if (e.cam < 0 || e.level || e.col < 0) continue;
                            const double* Wb = B.eD + (int64_t)k * LBA_EDGE_D + LE_W;
                            const double* xp = S.x + e.col * 6;
#pragma unroll
                            for (int m = 0; m < 3; m++) {
                                double s = 0.0;
#pragma unroll
                                for (int a = 0; a < 6; a++) s += Wb[a * 3 + m] * xp[a];
                                cl[m] -= s;
                            }
                        }
#pragma unroll
                        for (int m = 0; m < 3; m++) xl[m] = (PD[LP_DINV + m * 3] * cl[0] + PD[LP_DINV + m * 3 + 1] * cl[1]) + PD[LP_DINV + m * 3 + 2] * cl[2];
                    }
#pragma unroll
                    for (int m = 0; m < 3; m++) PD[LP_XT + m] = PD[LP_X + m] + xl[m];
                    sc += (xl[0] * (lambda * xl[0] + PD[LP_BL]) + xl[1] * (lambda * xl[1] + PD[LP_BL + 1])) + xl[2] * (lambda * xl[2] + PD[LP_BL + 2]);
                }
                const double scale = g2o_block_sum(S.part, sc);         // (its barriers publish the trial cameras)
                const double tempChi = lba_trial_chi2(S, B, W, nP, robust);
                if (g2o_lm_decide(lm, currentChi, tempChi, ok2, scale, rho)) {
                    for (int c = tid; c < nFree; c += LBA_T) { LbaCam& C = W.cams[S.freeCam[c]]; C.est = C.trial; }      // discardTop
                    for (int j = tid; j < nP; j += LBA_T) {
                        if (!B.pAct[W.ptList[j]]) continue;
                        double* PD = B.pD + (int64_t)W.ptList[j] * LBA_PT_D;
#pragma unroll
                        for (int m = 0; m < 3; m++) PD[LP_X + m] = PD[LP_XT + m];
                    }
                }                                                       // else pop: the estimates stay, the stored errors are the trial's (reading 6)
                __syncthreads();
                qmax++; trials[round]++;
            } while (g2o_lm_again(rho, qmax));
            if (g2o_lm_stop(lm, iniChi, currentChi, qmax, rho)) break;
        }
        if (status) break;
        if (round == 0 && B.rounds >= 2) {
            nLevel1 = lba_classify(S, B, W, nP, w, false);
            if (nLevel1 < 0) status = PGORB_LBA_NONFINITE;
            __syncthreads();
        }
    }
    if (!status) {
        nErase = lba_classify(S, B, W, nP, w, true);
        if (nErase < 0) status = PGORB_LBA_NONFINITE;
    }
    if (status == PGORB_LBA_NONFINITE && B.erase) {                      // the per-observation outputs of a window that ends here are 0
        __syncthreads();
        for (int j = tid; j < nP; j += LBA_T) {
            const int2 r = W.range[j];
            for (int k = r.x; k < r.y; k++) { const int64_t o = (int64_t)w * B.nobs + k; B.erase[o] = 0; B.chi2[o] = 0.0f; B.level[o] = 0; }
        }
    }
    // Recover optimized data (:759-777): SetPose(Converter::toCvMat(SE3quat)) for the local key frames, SetWorldPos for the local points
    for (int c = tid; c < nCam; c += LBA_T) {
        const LbaCam& C = W.cams[c];
        if (C.role != PGORB_LBA_ROLE_LOCAL) continue;
        pgorb_kf_pose o = B.pose[C.frame];
        if (!status) po_set_pose(C.est, o);
        B.poseOut[C.frame] = o;
    }
    if (!status)
        for (int j = tid; j < nP; j += LBA_T) {
            const int p = W.ptList[j];
            const double* PD = B.pD + (int64_t)p * LBA_PT_D;
#pragma unroll
            for (int m = 0; m < 3; m++) B.pts[p].pos[m] = __double2float_rn(PD[LP_X + m]);
        }
    if (tid == 0) {
        if (B.nErased) B.nErased[w] = status ? 0 : nErase;
        if (B.info) {
            int32_t* I = B.info + (int64_t)w * PGORB_LBA_INFO;
            const bool nf = status == PGORB_LBA_NONFINITE;
            I[0] = status; I[1] = H.nE; I[2] = H.nPts; I[3] = H.nLocal; I[4] = H.nFixed;
            I[5] = nf ? 0 : its[0]; I[6] = nf ? 0 : trials[0]; I[7] = nf ? 0 : its[1]; I[8] = nf ? 0 : trials[1]; I[9] = nf ? 0 : nLevel1;
        }
    }
}

static size_t lba_align(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" {

int pgorb_local_bundle_adjustment_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap,
        const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, const int32_t* d_kf_point, const uint8_t* d_kf_fixed_id0,
        const int32_t* d_win_start, const int32_t* d_win_kf, int nwin, int nwin_kf,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        const int32_t* d_obs_idx, int nobs, int rounds,
        pgorb_kf_pose* d_pose_out, uint8_t* d_erase, float* d_chi2, uint8_t* d_level, uint8_t* d_is_local, uint8_t* d_role,
        int32_t* d_info, int32_t* d_nerased, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || nwin < 0 || nwin_kf < 0 || npoints < 0 || nobs < 0 || rounds < 1 || rounds > 2 ||
        (nwin && (!d_win_start || !d_pose_out || !d_is_local || !d_role)) || (nwin_kf && !d_win_kf) ||
        (nframes && (!d_kps || !d_n || !d_pose || !d_kf_point)) || (npoints && (!d_points || !d_obs_start)) ||
        (nobs && (!d_obs_frame || !d_obs_idx)) || (nobs && nwin && (!d_erase || !d_chi2 || !d_level)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_local_bundle_adjustment_batch_device");
    if (cap > LBA_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_local_bundle_adjustment: more than 16000 keypoints per frame");
    if (!nwin) return 0;
    LbaBatch B;
    B.nlevels = pgorb_levels(c);
    memset(B.invSigma2, 0, sizeof(B.invSigma2));
    if (!(B.nlevels > 0) || B.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, nullptr, B.invSigma2) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    B.capP = std::max(1, std::min(npoints, PGORB_LBA_MAX_POINTS));
    B.capC = std::max(1, std::min(nframes, PGORB_LBA_MAX_LOCAL_KF + PGORB_LBA_MAX_FIXED_KF));
    B.capL = std::max(1, std::min(nframes, PGORB_LBA_MAX_LOCAL_KF));
    const size_t n6 = 6 * (size_t)B.capL;
    size_t o = lba_align(sizeof(LbaHdr));
    B.oPtList = o; o = lba_align(o + (size_t)B.capP * 4);
    B.oRange = o; o = lba_align(o + (size_t)B.capP * sizeof(int2));
    B.oCam = o; o = lba_align(o + (size_t)B.capC * sizeof(LbaCam));
    B.oHpp = o; o = lba_align(o + n6 * 6 * 8);
    B.oHs = o; o = lba_align(o + n6 * n6 * 8);
    B.oFrameCam = o; o = lba_align(o + (size_t)std::max(nframes, 1) * 4);
    B.capE = std::max(1, std::min(nobs, PGORB_LBA_MAX_EDGES));
    B.oCamStart = o; o = lba_align(o + (size_t)(B.capL + 1) * 4);
    B.oCamEdge = o; o = lba_align(o + (size_t)B.capE * sizeof(int2));
    B.winBytes = o;
    const size_t no = (size_t)std::max(nobs, 1), np = (size_t)std::max(npoints, 1);
    const size_t bEI = lba_align(no * sizeof(LbaEdgeI)), bED = lba_align(no * LBA_EDGE_D * 8), bPD = lba_align(np * LBA_PT_D * 8), bPA = lba_align(np * 4);
    void* scr;
    int rc = pg_ctx_scratch(c, bEI + bED + bPD + bPA + (size_t)nwin * B.winBytes, s, &scr);
    if (rc) return rc;
    uint8_t* a = (uint8_t*)scr;
    B.eI = (LbaEdgeI*)a; a += bEI; B.eD = (double*)a; a += bED; B.pD = (double*)a; a += bPD; B.pAct = (int32_t*)a; a += bPA; B.win = a;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.nframes = nframes; B.pose = d_pose; B.kfBad = d_kf_bad; B.kfPoint = d_kf_point; B.id0 = d_kf_fixed_id0;
    B.winStart = d_win_start; B.winKf = d_win_kf; B.nwin = nwin; B.nwinKf = nwin_kf;
    B.npoints = npoints; B.pts = d_points; B.ptBad = d_point_bad; B.obsStart = d_obs_start; B.obsFrame = d_obs_frame; B.obsIdx = d_obs_idx; B.nobs = nobs;
    B.rounds = rounds;
    B.poseOut = d_pose_out; B.erase = nobs ? d_erase : nullptr; B.chi2 = d_chi2; B.level = d_level; B.isLocal = d_is_local; B.role = d_role;
    B.info = d_info; B.nErased = d_nerased;
    if (nobs && (hipMemsetAsync(d_erase, 0, (size_t)nwin * nobs, s) != hipSuccess || hipMemsetAsync(d_chi2, 0, (size_t)nwin * nobs * 4, s) != hipSuccess ||
                 hipMemsetAsync(d_level, 0, (size_t)nwin * nobs, s) != hipSuccess))
        return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_lba_prepare, dim3((unsigned)nwin), dim3(LBA_T), 0, s, B);
    hipLaunchKernelGGL(k_lba, dim3((unsigned)nwin), dim3(LBA_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_lba_prepare / k_lba launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool lba_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

// host buffers: a one-window batch of the device form; the inputs are checked and the capacities counted here
int pgorb_local_bundle_adjustment(pgorb_ctx* c, int nkf, const pgorb_keypoint* const* kps, const int32_t* n, const pgorb_kf_pose* pose,
        const uint8_t* kf_bad, const int32_t* const* kf_point, const uint8_t* kf_fixed_id0, int nlocal, const int32_t* local_kf,
        int npoints, pgorb_map_point* points, const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame,
        const int32_t* obs_idx, int rounds, pgorb_kf_pose* pose_out, uint8_t* erase, float* chi2, uint8_t* level, uint8_t* is_local,
        uint8_t* role, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    int cap = 1, nobs = 0;
    if (nkf < 0 || nlocal < 0 || npoints < 0) why = "a count is negative";
    else if (rounds < 1 || rounds > 2) why = "rounds is neither 1 nor 2";
    else if (!obs_start || (nkf && (!kps || !n || !pose || !kf_point || !pose_out || !role)) || (nlocal && !local_kf) || (npoints && (!points || !is_local)))
        why = "an array that is read or written is NULL";
    for (int f = 0; !why && f < nkf; f++) {
        if (n[f] < 0 || (n[f] && (!kps[f] || !kf_point[f]))) why = "a key frame's count is negative or its arrays are NULL";
        else if (!lba_all_finite(pose[f].Tcw, 12) || !lba_all_finite(&pose[f].fx, 4)) why = "a pose or a camera is not finite";
        else if (pose[f].fx == 0.0f || pose[f].fy == 0.0f) why = "fx or fy is zero";
        else cap = std::max(cap, n[f]);
        for (int i = 0; !why && i < n[f]; i++)
            if (kf_point[f][i] < -1 || kf_point[f][i] >= npoints) why = "a slot's point index is out of range";
    }
    for (int i = 0; !why && i < nlocal; i++)
        if (local_kf[i] < 0 || local_kf[i] >= nkf) why = "a local key frame is out of range";
    if (!why && obs_start[0] != 0) why = "obs_start[0] must be 0";
    for (int p = 0; !why && p < npoints; p++) {
        if (obs_start[p + 1] < obs_start[p]) why = "obs_start decreases";
        else if (!lba_all_finite(points[p].pos, 3)) why = "a point is not finite";
    }
    if (!why) {
        nobs = obs_start[npoints];
        if (nobs && (!obs_frame || !obs_idx || !erase || !chi2 || !level)) why = "an array that is read or written is NULL";
    }
    std::vector<int32_t> seen((size_t)std::max(nkf, 1), -1);
    for (int p = 0; !why && p < npoints; p++)
        for (int k = obs_start[p]; !why && k < obs_start[p + 1]; k++) {
            const int f = obs_frame[k];
            if (f < 0 || f >= nkf || obs_idx[k] < 0 || obs_idx[k] >= n[f]) why = "an observation names a key frame or keypoint out of range";
            else if (seen[f] == p) why = "a list names a key frame twice";
            else if (kps[f][obs_idx[k]].octave < 0 || kps[f][obs_idx[k]].octave >= nlevels) why = "an octave is outside the context's levels";
            else seen[f] = p;
        }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_local_bundle_adjustment: ") + why).c_str());
    for (int f = 0; f < nkf; f++)
        if (n[f] > LBA_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_local_bundle_adjustment: more than 16000 keypoints per frame");
    {   // the capacities, counted as the device derives the sets
        std::vector<uint8_t> ro((size_t)std::max(nkf, 1), 0), loc((size_t)std::max(npoints, 1), 0);
        for (int i = 0; i < nlocal; i++) ro[local_kf[i]] = (kf_bad && kf_bad[local_kf[i]]) ? LBA_ROLE_LISTED_BAD : PGORB_LBA_ROLE_LOCAL;
        int nLoc = 0, nFix = 0, nPts = 0, nE = 0;
        for (int f = 0; f < nkf; f++) {
            if (ro[f] != PGORB_LBA_ROLE_LOCAL) continue;
            nLoc++;
            for (int i = 0; i < n[f]; i++) {
                const int p = kf_point[f][i];
                if (p >= 0 && !(point_bad && point_bad[p]) && !loc[p]) { loc[p] = 1; nPts++; }
            }
        }
        for (int p = 0; p < npoints; p++)
            for (int k = obs_start[p]; loc[p] && k < obs_start[p + 1]; k++) {
                const int f = obs_frame[k];
                if (kf_bad && kf_bad[f]) continue;
                nE++;
                if (ro[f] == 0) { ro[f] = PGORB_LBA_ROLE_FIXED; nFix++; }
            }
        if (nLoc > PGORB_LBA_MAX_LOCAL_KF) why = "more than 64 local key frames";
        else if (nFix > PGORB_LBA_MAX_FIXED_KF) why = "more than 256 fixed key frames";
        else if (nPts > PGORB_LBA_MAX_POINTS) why = "more than 8192 local points";
        else if (nE > PGORB_LBA_MAX_EDGES) why = "more than 65536 edges";
        if (why) return pg_ctx_fail(c, PGORB_E_LIMIT, (std::string("pgorb_local_bundle_adjustment: ") + why).c_str());
    }
    const int nf = std::max(nkf, 1), np = std::max(npoints, 1), no = std::max(nobs, 1), nl = std::max(nlocal, 1);
    const size_t kb = sizeof(pgorb_keypoint);
    PgHostCall s(c);
    const size_t oK = s.region(PG_UP, (size_t)nf * cap * kb), oN = s.region(PG_UP, (size_t)nf * 4), oPose = s.region(PG_UP, (size_t)nf * sizeof(pgorb_kf_pose)),
                 oKB = s.region(PG_UP, nf), oSl = s.region(PG_UP, (size_t)nf * cap * 4), oId = s.region(PG_UP, nf), oWS = s.region(PG_UP, 8),
                 oWK = s.region(PG_UP, (size_t)nl * 4), oB = s.region(PG_UP, np), oOS = s.region(PG_UP, (size_t)(npoints + 1) * 4),
                 oOF = s.region(PG_UP, (size_t)no * 4), oOI = s.region(PG_UP, (size_t)no * 4),
                 oP = s.region(PG_INOUT, (size_t)np * sizeof(pgorb_map_point)), oPO = s.region(PG_INOUT, (size_t)nf * sizeof(pgorb_kf_pose)),
                 oEr = s.region(PG_DOWN, no), oChi = s.region(PG_DOWN, (size_t)no * 4), oLv = s.region(PG_DOWN, no), oIL = s.region(PG_DOWN, np),
                 oRo = s.region(PG_DOWN, nf), oR = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    for (int f = 0; f < nkf; f++) {
        s.put(oK, kps[f], (size_t)n[f] * kb, (size_t)f * cap * kb, (size_t)cap * kb);
        memset(s.host(oSl) + (size_t)f * cap * 4, 0xFF, (size_t)cap * 4);
        s.put(oSl, kf_point[f], (size_t)n[f] * 4, (size_t)f * cap * 4);
    }
    s.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    s.put(oPose, pose, (size_t)nkf * sizeof(pgorb_kf_pose), 0, (size_t)nf * sizeof(pgorb_kf_pose));
    s.put(oKB, kf_bad, nkf, 0, nf);
    s.put(oId, kf_fixed_id0, nkf, 0, nf);
    const int32_t ws[2] = {0, nlocal};
    s.put(oWS, ws, 8);
    s.put(oWK, local_kf, (size_t)nlocal * 4, 0, (size_t)nl * 4);
    s.put(oB, point_bad, npoints, 0, np);
    s.put(oOS, obs_start, (size_t)(npoints + 1) * 4);
    s.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    s.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    s.put(oPO, pose, (size_t)nkf * sizeof(pgorb_kf_pose), 0, (size_t)nf * sizeof(pgorb_kf_pose));      // pose_out of a frame that is not local = its input
    int32_t* R = s.dev<int32_t>(oR);                                    // nerased, info[PGORB_LBA_INFO]
    if ((rc = s.run([&] {
            return pgorb_local_bundle_adjustment_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), nkf, cap, s.dev<pgorb_kf_pose>(oPose),
                    s.dev(oKB), s.dev<int32_t>(oSl), s.dev(oId), s.dev<int32_t>(oWS), s.dev<int32_t>(oWK), 1, nlocal, npoints,
                    s.dev<pgorb_map_point>(oP), s.dev(oB), s.dev<int32_t>(oOS), s.dev<int32_t>(oOF), s.dev<int32_t>(oOI), nobs, rounds,
                    s.dev<pgorb_kf_pose>(oPO), s.dev(oEr), s.dev<float>(oChi), s.dev(oLv), s.dev(oIL), s.dev(oRo), R + 1, R, nullptr); }))) return rc;
    memcpy(points, s.host(oP), (size_t)npoints * sizeof(pgorb_map_point));
    memcpy(pose_out, s.host(oPO), (size_t)nkf * sizeof(pgorb_kf_pose));
    if (nobs) { memcpy(erase, s.host(oEr), nobs); memcpy(chi2, s.host(oChi), (size_t)nobs * 4); memcpy(level, s.host(oLv), nobs); }
    if (npoints) memcpy(is_local, s.host(oIL), npoints);
    if (nkf) memcpy(role, s.host(oRo), nkf);
    const int32_t* r = s.host<int32_t>(oR);
    if (info) memcpy(info, r + 1, PGORB_LBA_INFO * 4);
    return r[0];
}

}  // extern "C"
