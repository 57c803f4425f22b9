// loop_correct.hip -- the two map rewrites of loop closing that sit between its numerical steps, on resident arrays, on gfx950.
//
// Restates (thirdparty/orb-slam2):
//   LoopClosing::CorrectLoop, the propagation          src/LoopClosing.cc:438-516 (without the UpdateConnections of :515)
//   LoopClosing::RunGlobalBundleAdjustment, the update  src/LoopClosing.cc:679-742
//   KeyFrame::SetPose, GetPoseInverse                  src/KeyFrame.cc:61-93
//   MapPoint::UpdateNormalAndDepth                     src/MapPoint.cc:347-388
// under the readings of DESIGN.md section 4 (loop_pose.h holds the ones shared with essential_graph.hip and map_point.hip).
//
// CorrectLoop.  The reference walks CorrectedSim3, a std::map keyed by KeyFrame*, and mnCorrectedByKF lets the first key frame in
// ADDRESS order that holds a point in a slot correct it.  Here:
//   k_lc_init      the outputs' defaults (pose_out = pose, no Sim3, no claim) and the scratch
//   k_lc_rank      the inverse of kf_order (address rank -> key frame), as k_cov_prep
//   k_lc_members   a thread per list entry (+ cur_kf): the two Sim3s and the corrected pose; an integer compare-and-swap makes a
//                  key frame named twice one member
//   k_lc_claim     a thread per (member, slot): atomicMin of the member's address rank into the point's claim -- a minimum has no
//                  order, and no floating-point atomic is used
//   k_lc_points    a thread per point: the claimed ones are mapped and get UpdateNormalAndDepth in the state the reference is in at
//                  that moment (the members of a smaller rank already have their corrected centre, the corrector itself not yet)
// The map update after global bundle adjustment.  The reference walks the spanning tree breadth first from the origins; a child
// that was not adjusted takes (Tchild * Twc_parent) * TcwGBA_parent with both operands of the first product taken before the
// update, so its result is a function of the chain down from its nearest adjusted ancestor alone, multiplied in that order:
//   k_mu_kf        a thread per key frame walks up to the origin (bounded by nframes: a cycle is not visited), then multiplies down
//                  its own chain; no launch count depends on the tree's depth
//   k_mu_points    a thread per point
#include "kf_window.h"                     // kf_row, kf_to_camera: Rcw*p + tcw
#include "loop_pose.h"
#include <math.h>
#include <string>
#include <vector>

#define LC_T 256
#define LC_NONE 0x7FFFFFFF

struct LcArgs {
    const pgorb_keypoint* K; const int32_t* n; int nframes, cap; const pgorb_kf_pose* pose; int curKf; const OsSim* scw;
    int nlist; const int32_t* list; const int32_t* nlistDev; const int32_t* order; const int32_t* kfPoint;
    int npoints; pgorb_map_point* pts; const uint8_t* pbad; const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs;
    const int32_t* refObs; const int32_t* refKf;
    uint8_t* hasCor; OsSim* cor; uint8_t* hasNon; OsSim* non; pgorb_kf_pose* poseOut; int32_t* correctedBy; int32_t* pointRefKf; int32_t* info;
    int32_t* inv; int32_t* memberRank; int32_t* claim;                               // the arena
    float sf[PG_MAXL + 1]; int nlevels;
};
static_assert(sizeof(OsSim) == sizeof(pgorb_sim3d), "pgorb_sim3d is g2o::Sim3's r, t, s");

// the address rank of key frame f, or -1 when kf_order gives it none of its own (the contract of the covisibility block)
__device__ __forceinline__ int lc_rank(const LcArgs& A, int f)
{
    if (!A.order) return f;
    const int r = A.order[f];
    return (r >= 0 && r < A.nframes && A.inv[r] == f) ? r : -1;
}
// entry g of the member list: d_list, then cur_kf; -1 = no member
__device__ __forceinline__ int lc_entry(const LcArgs& A, int g)
{
    const int cur = A.curKf;
    if (cur < 0 || cur >= A.nframes) return -1;
    if (g == A.nlist) return cur;
    if (A.nlistDev && g >= *A.nlistDev) return -1;                                    // past the row's count: stale entries, not padding
    const int f = A.list[g];
    return (f < 0 || f >= A.nframes || f == cur) ? -1 : f;
}

__global__ __launch_bounds__(LC_T) void k_lc_init(LcArgs A)
{
    const int64_t g = (int64_t)blockIdx.x * LC_T + threadIdx.x;
    if (g < A.nframes) {
        OsSim Z;
        memset(&Z, 0, sizeof(Z));
        A.inv[g] = -1; A.memberRank[g] = -1;
        A.hasCor[g] = 0; A.hasNon[g] = 0; A.cor[g] = Z; A.non[g] = Z;
        A.poseOut[g] = A.pose[g];
    }
    if (g < A.npoints) A.claim[g] = LC_NONE;
    if (g < PGORB_LC_INFO) A.info[g] = 0;
}

__global__ __launch_bounds__(LC_T) void k_lc_rank(LcArgs A)
{
    const int t = blockIdx.x * LC_T + threadIdx.x;
    if (t < A.nframes) {
        const int r = A.order[t];
        if (r >= 0 && r < A.nframes) atomicMax(&A.inv[r], t);                         // a rank named twice belongs to the larger index
    }
}

__global__ __launch_bounds__(LC_T) void k_lc_members(LcArgs A)
{
    const int g = blockIdx.x * LC_T + threadIdx.x;
    if (g > A.nlist) return;
    const int f = lc_entry(A, g), cur = A.curKf;
    if (f < 0 || lc_rank(A, cur) < 0) return;
    const int rank = lc_rank(A, f);
    if (rank < 0) return;
    if (atomicCAS(&A.memberRank[f], -1, rank) != -1) return;                          // named before
    atomicAdd(&A.info[1], 1);
    const pgorb_kf_pose P = A.pose[f];
    const OsSim scw = *A.scw;
    OsSim C;
    if (f == cur) C = scw;                                                            // CorrectedSim3[mpCurrentKF] = mg2oScw (:439)
    else {
        float Twc[12], Tic[12];
        lp_twc(A.pose[cur], Twc);                                                     // mpCurrentKF->GetPoseInverse() (:440)
        lp_mul44(P.Tcw, Twc, Tic);                                                    // Tic = Tiw*Twc (:455)
        C = os_mul(lp_sim3_from_pose(Tic), scw);                                      // g2oSic*mg2oScw (:458-459)
    }
    A.cor[f] = C; A.hasCor[f] = 1;
    A.non[f] = lp_sim3_from_pose(P.Tcw); A.hasNon[f] = 1;                             // :464-468
    pgorb_kf_pose o = P;
    lp_pose_from_sim3(C, o);                                                          // :504-512
    A.poseOut[f] = o;
}

__global__ __launch_bounds__(LC_T) void k_lc_claim(LcArgs A)
{
    const int s = blockIdx.x * LC_T + threadIdx.x;
    const int f = lc_entry(A, blockIdx.y);
    if (f < 0) return;
    const int rank = A.memberRank[f];
    if (rank < 0 || s >= min(max(A.n[f], 0), A.cap)) return;
    const int p = A.kfPoint[(int64_t)f * A.cap + s];
    if (p < 0 || p >= A.npoints || (A.pbad && A.pbad[p])) return;                     // :484-487
    atomicMin(&A.claim[p], rank);
}

__global__ __launch_bounds__(LC_T) void k_lc_points(LcArgs A)
{
    const int p = blockIdx.x * LC_T + threadIdx.x;
    if (p >= A.npoints) return;
    const int rk = A.claim[p];
    const int by = rk == LC_NONE ? -1 : (A.order ? A.inv[rk] : rk);
    A.correctedBy[p] = by;
    A.pointRefKf[p] = by >= 0 ? by : (A.refKf ? A.refKf[p] : -1);
    if (by < 0) return;
    atomicAdd(&A.info[2], 1);
    float pos[3];
    {
        const float* in = A.pts[p].pos;
        double x, y, z, X, Y, Z;
        lp_map(A.non[by], (double)in[0], (double)in[1], (double)in[2], x, y, z);      // g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw)) (:494)
        lp_map(os_inverse(A.cor[by]), x, y, z, X, Y, Z);
        pos[0] = __double2float_rn(X); pos[1] = __double2float_rn(Y); pos[2] = __double2float_rn(Z);
        A.pts[p].pos[0] = pos[0]; A.pts[p].pos[1] = pos[1]; A.pts[p].pos[2] = pos[2];
    }
    // UpdateNormalAndDepth (:500)
    const int a = A.obsStart[p], b = A.obsStart[p + 1];
    if (a < 0 || b < a || b > A.nobs) { atomicOr(&A.info[0], PGORB_LC_BAD_INDEX); return; }
    const int n = b - a;
    if (n == 0) return;                                                               // MapPoint.cc:362-363
    if (n > PGORB_MP_MAX_OBS) { atomicOr(&A.info[0], PGORB_LC_OVER_OBS); atomicAdd(&A.info[3], 1); return; }
    const int r = A.refObs[p];
    bool ok = r >= 0 && r < n;
    for (int l = 0; ok && l < n; l++) {
        const int f = A.obsFrame[a + l], i = A.obsIdx[a + l];
        ok = f >= 0 && f < A.nframes && i >= 0 && i < min(max(A.n[f], 0), A.cap);
    }
    if (!ok) { atomicOr(&A.info[0], PGORB_LC_BAD_INDEX); return; }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int l = 0; l < n; l++) {
        const int f = A.obsFrame[a + l];
        const int fr = A.memberRank[f];
        // a member of a smaller address rank has had its SetPose (:512); the corrector's own comes after this loop
        const float* Ow = (fr >= 0 && fr < rk) ? A.poseOut[f].Ow : A.pose[f].Ow;
        float t[3];
        double nd;
        mp_term(pos, Ow, t, nd);
        sx = __fadd_rn(sx, t[0]); sy = __fadd_rn(sy, t[1]); sz = __fadd_rn(sz, t[2]);
        if (l == r) {
            float mn, mx;
            mp_depth(A.sf, A.nlevels, nd, A.K[(int64_t)f * A.cap + A.obsIdx[a + l]].octave, mn, mx);
            A.pts[p].min_distance = mn; A.pts[p].max_distance = mx;
        }
    }
    const float sc = cnm_f(__ddiv_rn(1.0, (double)n));
    A.pts[p].normal[0] = __fmul_rn(sx, sc); A.pts[p].normal[1] = __fmul_rn(sy, sc); A.pts[p].normal[2] = __fmul_rn(sz, sc);
}

struct MuArgs {
    int nframes; const pgorb_kf_pose* pose; const pgorb_kf_pose* poseGba; const uint8_t* kfDone; const int32_t* parent;
    const uint8_t* origin; const uint8_t* kfBad;
    int npoints; pgorb_map_point* pts; const float* posGba; const uint8_t* pointDone; const uint8_t* pbad; const int32_t* refKf;
    pgorb_kf_pose* poseOut; uint8_t* kfUpdated; uint8_t* pointUpdated; int32_t* info;
};

__device__ __forceinline__ bool mu_bad(const MuArgs& M, int k) { return M.kfBad && M.kfBad[k]; }

__global__ __launch_bounds__(LC_T) void k_mu_kf(MuArgs M)
{
    const int k = blockIdx.x * LC_T + threadIdx.x;
    if (k >= M.nframes) return;
    pgorb_kf_pose out = M.pose[k];
    int upd = 0;
    if (!mu_bad(M, k)) {
        // up: the nearest adjusted key frame of the chain (k itself included), and whether the chain reaches an origin
        int cur = k, steps = 0, doneDepth = -1, doneKf = -1;
        bool reached = false;
        for (;;) {
            if (doneKf < 0 && M.kfDone[cur]) { doneKf = cur; doneDepth = steps; }
            if (M.origin[cur]) { reached = true; break; }
            const int p = M.parent[cur];
            if (p < 0 || p >= M.nframes || mu_bad(M, p)) break;
            if (++steps >= M.nframes) break;                                          // more key frames than there are: a cycle
            cur = p;
        }
        if (reached && doneKf >= 0) {
            upd = 1;
            if (doneDepth == 0) out = M.poseGba[k];                                   // SetPose(mTcwGBA) of an adjusted key frame (:701)
            else {
                float T[12];
#pragma unroll
                for (int q = 0; q < 12; q++) T[q] = M.poseGba[doneKf].Tcw[q];
                for (int lvl = doneDepth - 1; lvl >= 0; lvl--) {                      // down: the child at depth lvl of k's chain
                    int c = k;
                    for (int h = 0; h < lvl; h++) c = M.parent[c];
                    float Twc[12], Tcc[12], Tn[12];
                    lp_twc(M.pose[M.parent[c]], Twc);                                 // pKF->GetPoseInverse() before its SetPose (:686)
                    lp_mul44(M.pose[c].Tcw, Twc, Tcc);                                // Tchildc = pChild->GetPose()*Twc (:692)
                    lp_mul44(Tcc, T, Tn);                                             // pChild->mTcwGBA = Tchildc*pKF->mTcwGBA (:693)
#pragma unroll
                    for (int q = 0; q < 12; q++) T[q] = Tn[q];
                }
#pragma unroll
                for (int q = 0; q < 12; q++) out.Tcw[q] = T[q];
                po_set_ow(out);
                atomicAdd(&M.info[2], 1);
            }
            atomicAdd(&M.info[1], 1);
        }
    }
    M.poseOut[k] = out;
    M.kfUpdated[k] = (uint8_t)upd;
}

__global__ __launch_bounds__(LC_T) void k_mu_points(MuArgs M)
{
    const int p = blockIdx.x * LC_T + threadIdx.x;
    if (p >= M.npoints) return;
    int upd = 0;
    if (!(M.pbad && M.pbad[p])) {                                                     // :712-713
        float* pos = M.pts[p].pos;
        if (M.pointDone[p]) {                                                         // :715-719
            pos[0] = M.posGba[(int64_t)p * 3]; pos[1] = M.posGba[(int64_t)p * 3 + 1]; pos[2] = M.posGba[(int64_t)p * 3 + 2];
            upd = 1;
        } else {
            const int r = M.refKf[p];
            if (r >= 0 && r < M.nframes && M.kfUpdated[r]) {                          // :723-726
                float Xc[3], w[3];
                kf_to_camera(M.pose[r], pos, Xc);                                   // Rcw*pos + tcw of mTcwBefGBA (:729-731)
                const pgorb_kf_pose& N = M.poseOut[r];
#pragma unroll
                for (int c = 0; c < 3; c++) {                                         // Rwc*Xc + twc of GetPoseInverse() (:734-738)
                    const float col[3] = {N.Tcw[c], N.Tcw[4 + c], N.Tcw[8 + c]};
                    w[c] = kf_row(col, N.Ow[c], Xc);
                }
                pos[0] = w[0]; pos[1] = w[1]; pos[2] = w[2];
                upd = 1;
            }
        }
        if (upd) atomicAdd(&M.info[3], 1);
    }
    M.pointUpdated[p] = (uint8_t)upd;
}

extern "C" {

int pgorb_correct_loop_poses_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap,
        const pgorb_kf_pose* d_pose, int cur_kf, const pgorb_sim3d* d_scw, int nlist, const int32_t* d_list, const int32_t* d_list_count,
        const int32_t* d_kf_order, const int32_t* d_kf_point, int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start,
        const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs, const int32_t* d_ref_obs, const int32_t* d_ref_kf,
        uint8_t* d_has_corrected, pgorb_sim3d* d_corrected, uint8_t* d_has_non_corrected, pgorb_sim3d* d_non_corrected,
        pgorb_kf_pose* d_pose_out, int32_t* d_corrected_by, int32_t* d_point_ref_kf, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || nlist < 0 || npoints < 0 || nobs < 0 || !d_info || !d_scw || (nlist && !d_list) ||
        (nframes && (!d_kps || !d_n || !d_pose || !d_kf_point || !d_has_corrected || !d_corrected || !d_has_non_corrected || !d_non_corrected ||
                     !d_pose_out || d_pose_out == d_pose)) ||
        (npoints && (!d_points || !d_obs_start || !d_ref_obs || !d_ref_kf || !d_corrected_by || !d_point_ref_kf)) || (nobs && (!d_obs_frame || !d_obs_idx)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_correct_loop_poses_device");
    if (nframes > PGORB_COVIS_MAX_KF || nlist > PGORB_COVIS_MAX_KF)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_correct_loop_poses: more than PGORB_COVIS_MAX_KF key frames or list entries");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    LcArgs A;
    memset(&A, 0, sizeof(A));
    A.K = d_kps; A.n = d_n; A.nframes = nframes; A.cap = cap; A.pose = d_pose; A.curKf = cur_kf; A.scw = (const OsSim*)d_scw;
    A.nlist = nlist; A.list = d_list; A.nlistDev = d_list_count; A.order = d_kf_order; A.kfPoint = d_kf_point;
    A.npoints = npoints; A.pts = d_points; A.pbad = d_point_bad; A.obsStart = d_obs_start; A.obsFrame = d_obs_frame; A.obsIdx = d_obs_idx;
    A.nobs = nobs; A.refObs = d_ref_obs; A.refKf = d_ref_kf;
    A.hasCor = d_has_corrected; A.cor = (OsSim*)d_corrected; A.hasNon = d_has_non_corrected; A.non = (OsSim*)d_non_corrected;
    A.poseOut = d_pose_out; A.correctedBy = d_corrected_by; A.pointRefKf = d_point_ref_kf; A.info = d_info;
    pgorb_scale_tables(c, A.sf, nullptr, nullptr, nullptr);
    A.nlevels = pgorb_levels(c);
    if (A.nlevels < 1) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    PgCarve carve;
    const size_t oInv = carve.take((size_t)std::max(nframes, 1) * 4), oMem = carve.take((size_t)std::max(nframes, 1) * 4),
                 oClaim = carve.take((size_t)std::max(npoints, 1) * 4);
    void* scr;
    int rc = pg_ctx_scratch(c, carve.o, s, &scr);
    if (rc) return rc;
    A.inv = (int32_t*)((uint8_t*)scr + oInv); A.memberRank = (int32_t*)((uint8_t*)scr + oMem); A.claim = (int32_t*)((uint8_t*)scr + oClaim);
    const int64_t items = std::max<int64_t>(std::max(nframes, npoints), PGORB_LC_INFO);
    hipLaunchKernelGGL(k_lc_init, dim3((unsigned)((items + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, A);
    if (nframes) {
        if (d_kf_order) hipLaunchKernelGGL(k_lc_rank, dim3((unsigned)((nframes + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, A);
        hipLaunchKernelGGL(k_lc_members, dim3((unsigned)((nlist + 1 + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, A);
        if (npoints) hipLaunchKernelGGL(k_lc_claim, dim3((unsigned)((cap + LC_T - 1) / LC_T), (unsigned)(nlist + 1)), dim3(LC_T), 0, s, A);
    }
    if (npoints) hipLaunchKernelGGL(k_lc_points, dim3((unsigned)((npoints + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, A);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "a loop-correction launch failed");
    return pg_ctx_scratch_done(c, s);
}

int pgorb_global_ba_map_update_device(pgorb_ctx* c, int nframes, const pgorb_kf_pose* d_pose, const pgorb_kf_pose* d_pose_gba,
        const uint8_t* d_kf_done, const int32_t* d_parent, const uint8_t* d_kf_origin, const uint8_t* d_kf_bad, int npoints,
        pgorb_map_point* d_points, const float* d_pos_gba, const uint8_t* d_point_done, const uint8_t* d_point_bad, const int32_t* d_ref_kf,
        pgorb_kf_pose* d_pose_out, uint8_t* d_kf_updated, uint8_t* d_point_updated, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || npoints < 0 || !d_info ||
        (nframes && (!d_pose || !d_pose_gba || !d_kf_done || !d_parent || !d_kf_origin || !d_pose_out || !d_kf_updated || d_pose_out == d_pose)) ||
        (npoints && (!d_points || !d_pos_gba || !d_point_done || !d_ref_kf || !d_point_updated)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_global_ba_map_update_device");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_ba_map_update: more than PGORB_COVIS_MAX_KF key frames");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const MuArgs M = {nframes, d_pose, d_pose_gba, d_kf_done, d_parent, d_kf_origin, d_kf_bad, npoints, d_points, d_pos_gba, d_point_done,
                      d_point_bad, d_ref_kf, d_pose_out, d_kf_updated, d_point_updated, d_info};
    if (hipMemsetAsync(d_info, 0, PGORB_MU_INFO * 4, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (nframes) hipLaunchKernelGGL(k_mu_kf, dim3((unsigned)((nframes + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, M);
    if (npoints) hipLaunchKernelGGL(k_mu_points, dim3((unsigned)((npoints + LC_T - 1) / LC_T)), dim3(LC_T), 0, s, M);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_mu_kf / k_mu_points launch failed");
    return 0;
}

// ---- the host forms: checked, then one synchronous call of the device form
static bool lc_pose_finite(const pgorb_kf_pose& P)
{
    for (int k = 0; k < 12; k++) if (!std::isfinite(P.Tcw[k])) return false;
    return std::isfinite(P.Ow[0]) && std::isfinite(P.Ow[1]) && std::isfinite(P.Ow[2]);
}
static bool lc_pos_finite(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

int pgorb_correct_loop_poses(pgorb_ctx* c, int nkf, const pgorb_keypoint* const* kps, const int32_t* n, const pgorb_kf_pose* pose, int cur_kf,
        const pgorb_sim3d* scw, int nlist, const int32_t* list, const int32_t* kf_order, const int32_t* const* kf_point, int npoints,
        pgorb_map_point* points, const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx,
        const int32_t* ref_obs, const int32_t* ref_kf, uint8_t* has_corrected, pgorb_sim3d* corrected, uint8_t* has_non_corrected,
        pgorb_sim3d* non_corrected, pgorb_kf_pose* pose_out, int32_t* corrected_by, int32_t* point_ref_kf, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const std::string fn = "pgorb_correct_loop_poses: ";
    const char* why = nullptr;
    if (nkf < 0 || nlist < 0 || npoints < 0) why = "a count is negative";
    else if (!scw || !info || (nlist && !list) || !obs_start ||
             (nkf && (!kps || !n || !pose || !kf_point || !has_corrected || !corrected || !has_non_corrected || !non_corrected || !pose_out)) ||
             (npoints && (!points || !ref_obs || !ref_kf || !corrected_by || !point_ref_kf)))
        why = "an array that is read or written is NULL";
    else if (cur_kf < 0 || cur_kf >= nkf) why = "cur_kf is out of range";
    else if (pose_out == pose) why = "pose_out must not be pose";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    if (nkf > PGORB_COVIS_MAX_KF || nlist > PGORB_COVIS_MAX_KF)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_correct_loop_poses: more than PGORB_COVIS_MAX_KF key frames or list entries");
    int cap = 1;
    for (int k = 0; k < nkf; k++) {
        if (n[k] < 0 || (n[k] && (!kps[k] || !kf_point[k]))) return pg_ctx_fail(c, PGORB_E_ARG, (fn + "an array that is read or written is NULL").c_str());
        if (n[k] > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        cap = std::max(cap, n[k]);
    }
    for (int k = 0; !why && k < nkf; k++) {
        if (!lc_pose_finite(pose[k])) why = "a pose is not finite";
        for (int s = 0; !why && s < n[k]; s++)
            if (kf_point[k][s] < -1 || kf_point[k][s] >= npoints) why = "a slot names a point out of range";
    }
    if (!why) {
        for (int k = 0; k < 4; k++) if (!std::isfinite(scw->r[k])) why = "scw is not finite";
        for (int k = 0; k < 3; k++) if (!std::isfinite(scw->t[k])) why = "scw is not finite";
        if (!std::isfinite(scw->s)) why = "scw is not finite";
        else if (!why && !(scw->s > 0.0)) why = "the scale of scw is not positive";
    }
    if (!why && kf_order) {
        std::vector<uint8_t> seen((size_t)nkf, 0);
        for (int k = 0; !why && k < nkf; k++) {
            if (kf_order[k] < 0 || kf_order[k] >= nkf || seen[kf_order[k]]) why = "kf_order is not a permutation";
            else seen[kf_order[k]] = 1;
        }
    }
    if (!why && obs_start[0] != 0) why = "obs_start[0] must be 0";
    for (int p = 0; !why && p < npoints; p++)
        if (obs_start[p + 1] < obs_start[p]) why = "obs_start decreases";
    const int nobs = why ? 0 : obs_start[npoints];
    if (!why && nobs && (!obs_frame || !obs_idx)) why = "an array that is read or written is NULL";
    for (int o = 0; !why && o < nobs; o++)
        if (obs_frame[o] < 0 || obs_frame[o] >= nkf || obs_idx[o] < 0 || obs_idx[o] >= n[obs_frame[o]]) why = "an observation names a key frame or keypoint out of range";
    if (!why) {
        std::vector<int32_t> seen((size_t)nkf, -1);
        for (int p = 0; !why && p < npoints; p++)
            for (int o = obs_start[p]; !why && o < obs_start[p + 1]; o++) {
                if (seen[obs_frame[o]] == p) why = "a list names a key frame twice";
                seen[obs_frame[o]] = p;
            }
    }
    for (int p = 0; !why && p < npoints; p++) {
        const int len = obs_start[p + 1] - obs_start[p];
        if (!lc_pos_finite(points[p].pos)) why = "a point is not finite";
        else if (ref_kf[p] < -1 || ref_kf[p] >= nkf) why = "ref_kf is out of range";
        else if (!(point_bad && point_bad[p]) && len > 0 && len <= PGORB_MP_MAX_OBS && (ref_obs[p] < 0 || ref_obs[p] >= len)) why = "ref_obs lies outside the point's list";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    const size_t K = (size_t)nkf, NP = (size_t)std::max(npoints, 1), NO = (size_t)std::max(nobs, 1), NL = (size_t)std::max(nlist, 1);
    const size_t kb = sizeof(pgorb_keypoint), pb = sizeof(pgorb_kf_pose);
    PgHostCall s(c);
    const size_t oK = s.region(PG_UP, K * cap * kb), oN = s.region(PG_UP, K * 4), oPose = s.region(PG_UP, K * pb), oScw = s.region(PG_UP, 64),
                 oList = s.region(PG_UP, NL * 4), oOrd = s.region(PG_UP, K * 4), oS = s.region(PG_UP, K * cap * 4), oB = s.region(PG_UP, NP),
                 oOS = s.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = s.region(PG_UP, NO * 4), oOI = s.region(PG_UP, NO * 4),
                 oRO = s.region(PG_UP, NP * 4), oRK = s.region(PG_UP, NP * 4), oPts = s.region(PG_INOUT, NP * sizeof(pgorb_map_point)),
                 oHc = s.region(PG_DOWN, K), oCor = s.region(PG_DOWN, K * 64), oHn = s.region(PG_DOWN, K), oNon = s.region(PG_DOWN, K * 64),
                 oPo = s.region(PG_DOWN, K * pb), oBy = s.region(PG_DOWN, NP * 4), oPr = s.region(PG_DOWN, NP * 4), oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    memset(s.host(oK), 0, K * cap * kb);
    for (int k = 0; k < nkf; k++) {
        if (n[k]) memcpy(s.host<pgorb_keypoint>(oK) + (size_t)k * cap, kps[k], (size_t)n[k] * kb);
        for (int q = 0; q < cap; q++) s.host<int32_t>(oS)[(size_t)k * cap + q] = q < n[k] ? kf_point[k][q] : -1;
    }
    s.put(oN, n, K * 4); s.put(oPose, pose, K * pb); s.put(oScw, scw, 64);
    s.put(oList, list, (size_t)nlist * 4, 0, NL * 4);
    s.put(oOrd, kf_order, K * 4, 0, K * 4);
    s.put(oB, point_bad, (size_t)npoints, 0, NP);
    s.put(oOS, obs_start, (size_t)(npoints + 1) * 4);
    s.put(oOF, obs_frame, (size_t)nobs * 4, 0, NO * 4); s.put(oOI, obs_idx, (size_t)nobs * 4, 0, NO * 4);
    s.put(oRO, ref_obs, (size_t)npoints * 4, 0, NP * 4); s.put(oRK, ref_kf, (size_t)npoints * 4, 0, NP * 4);
    s.put(oPts, points, (size_t)npoints * sizeof(pgorb_map_point), 0, NP * sizeof(pgorb_map_point));
    if ((rc = s.run([&] {
            return pgorb_correct_loop_poses_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), nkf, cap, s.dev<pgorb_kf_pose>(oPose), cur_kf,
                s.dev<pgorb_sim3d>(oScw), nlist, s.dev<int32_t>(oList), nullptr, kf_order ? s.dev<int32_t>(oOrd) : nullptr, s.dev<int32_t>(oS), npoints,
                s.dev<pgorb_map_point>(oPts), point_bad ? s.dev(oB) : nullptr, s.dev<int32_t>(oOS), s.dev<int32_t>(oOF), s.dev<int32_t>(oOI), nobs,
                s.dev<int32_t>(oRO), s.dev<int32_t>(oRK), s.dev(oHc), s.dev<pgorb_sim3d>(oCor), s.dev(oHn), s.dev<pgorb_sim3d>(oNon),
                s.dev<pgorb_kf_pose>(oPo), s.dev<int32_t>(oBy), s.dev<int32_t>(oPr), s.dev<int32_t>(oInfo), nullptr); }))) return rc;
    memcpy(has_corrected, s.host(oHc), K); memcpy(corrected, s.host(oCor), K * 64);
    memcpy(has_non_corrected, s.host(oHn), K); memcpy(non_corrected, s.host(oNon), K * 64);
    memcpy(pose_out, s.host(oPo), K * pb);
    if (npoints) {
        memcpy(points, s.host(oPts), (size_t)npoints * sizeof(pgorb_map_point));
        memcpy(corrected_by, s.host(oBy), (size_t)npoints * 4); memcpy(point_ref_kf, s.host(oPr), (size_t)npoints * 4);
    }
    memcpy(info, s.host(oInfo), PGORB_LC_INFO * 4);
    return info[2];
}

int pgorb_global_ba_map_update(pgorb_ctx* c, int nkf, const pgorb_kf_pose* pose, const pgorb_kf_pose* pose_gba, const uint8_t* kf_done,
        const int32_t* parent, const uint8_t* kf_origin, const uint8_t* kf_bad, int npoints, pgorb_map_point* points, const float* pos_gba,
        const uint8_t* point_done, const uint8_t* point_bad, const int32_t* ref_kf, pgorb_kf_pose* pose_out, uint8_t* kf_updated,
        uint8_t* point_updated, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const std::string fn = "pgorb_global_ba_map_update: ";
    const char* why = nullptr;
    if (nkf < 0 || npoints < 0) why = "a count is negative";
    else if (!info || (nkf && (!pose || !pose_gba || !kf_done || !parent || !kf_origin || !pose_out || !kf_updated)) ||
             (npoints && (!points || !pos_gba || !point_done || !ref_kf || !point_updated)))
        why = "an array that is read or written is NULL";
    else if (nkf && pose_out == pose) why = "pose_out must not be pose";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    if (nkf > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_ba_map_update: more than PGORB_COVIS_MAX_KF key frames");
    for (int k = 0; !why && k < nkf; k++) {
        if (parent[k] < -1 || parent[k] >= nkf) why = "a parent is out of range";
        else if (!lc_pose_finite(pose[k]) || (kf_done[k] && !lc_pose_finite(pose_gba[k]))) why = "a pose is not finite";
    }
    if (!why) {                                                                       // a parent cycle: colour the chains
        std::vector<int32_t> mark((size_t)nkf, -1);
        for (int k = 0; !why && k < nkf; k++) {
            int cur = k;
            while (cur >= 0 && mark[cur] < 0) { mark[cur] = k; cur = parent[cur]; }
            if (cur >= 0 && mark[cur] == k) why = "the parents form a cycle";
        }
    }
    for (int p = 0; !why && p < npoints; p++) {
        if (ref_kf[p] < -1 || ref_kf[p] >= nkf) why = "ref_kf is out of range";
        else if (!lc_pos_finite(points[p].pos) || (point_done[p] && !lc_pos_finite(pos_gba + (size_t)p * 3))) why = "a point is not finite";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (fn + why).c_str());
    const size_t K = (size_t)std::max(nkf, 1), NP = (size_t)std::max(npoints, 1), pb = sizeof(pgorb_kf_pose);
    PgHostCall s(c);
    const size_t oPose = s.region(PG_UP, K * pb), oGba = s.region(PG_UP, K * pb), oKd = s.region(PG_UP, K), oPar = s.region(PG_UP, K * 4),
                 oOr = s.region(PG_UP, K), oKb = s.region(PG_UP, K), oPg = s.region(PG_UP, NP * 12), oPd = s.region(PG_UP, NP),
                 oPb = s.region(PG_UP, NP), oRk = s.region(PG_UP, NP * 4), oPts = s.region(PG_INOUT, NP * sizeof(pgorb_map_point)),
                 oPo = s.region(PG_DOWN, K * pb), oKu = s.region(PG_DOWN, K), oPu = s.region(PG_DOWN, NP), oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oPose, pose, (size_t)nkf * pb, 0, K * pb); s.put(oGba, pose_gba, (size_t)nkf * pb, 0, K * pb);
    s.put(oKd, kf_done, (size_t)nkf, 0, K); s.put(oPar, parent, (size_t)nkf * 4, 0, K * 4); s.put(oOr, kf_origin, (size_t)nkf, 0, K);
    s.put(oKb, kf_bad, (size_t)nkf, 0, K);
    s.put(oPg, pos_gba, (size_t)npoints * 12, 0, NP * 12); s.put(oPd, point_done, (size_t)npoints, 0, NP);
    s.put(oPb, point_bad, (size_t)npoints, 0, NP); s.put(oRk, ref_kf, (size_t)npoints * 4, 0, NP * 4);
    s.put(oPts, points, (size_t)npoints * sizeof(pgorb_map_point), 0, NP * sizeof(pgorb_map_point));
    if ((rc = s.run([&] {
            return pgorb_global_ba_map_update_device(c, nkf, s.dev<pgorb_kf_pose>(oPose), s.dev<pgorb_kf_pose>(oGba), s.dev(oKd), s.dev<int32_t>(oPar),
                s.dev(oOr), kf_bad ? s.dev(oKb) : nullptr, npoints, s.dev<pgorb_map_point>(oPts), s.dev<float>(oPg), s.dev(oPd),
                point_bad ? s.dev(oPb) : nullptr, s.dev<int32_t>(oRk), s.dev<pgorb_kf_pose>(oPo), s.dev(oKu), s.dev(oPu), s.dev<int32_t>(oInfo),
                nullptr); }))) return rc;
    if (nkf) { memcpy(pose_out, s.host(oPo), (size_t)nkf * pb); memcpy(kf_updated, s.host(oKu), (size_t)nkf); }
    if (npoints) { memcpy(points, s.host(oPts), (size_t)npoints * sizeof(pgorb_map_point)); memcpy(point_updated, s.host(oPu), (size_t)npoints); }
    memcpy(info, s.host(oInfo), PGORB_MU_INFO * 4);
    return info[1];
}

}  // extern "C"
