// pnp.hip -- PnPsolver on gfx950: the RANSAC EPnP of a relocalisation candidate's matches, every hypothesis of the call's window
// evaluated at once and the reference's sequential stop rule (with its Refine) applied afterwards.
//
// Restates (thirdparty/orb-slam2):
//   PnPsolver::PnPsolver                          src/PnPsolver.cc:67-110 (the correspondences, in keypoint order)
//   PnPsolver::SetRansacParameters                :121-157 (on the host: pg_pnp_ransac, a table per N in the context)
//   PnPsolver::iterate / find                     :159-258 (the loop condition is an OR: a call's window is max(cap - first, n))
//   PnPsolver::Refine                             :260-305 (on the BEST set; true only for refined > min)
//   PnPsolver::CheckInliers                       :308-339 (its mixed float / double types)
//   compute_pose and everything it calls          :375-950 (pnp_epnp.h)
//   DUtils::Random::RandomInt                     DUtils/Random.cpp:47-50
//   Tracking::Relocalization                      src/Tracking.cc:1405-1420 (pose_out, kp_point_out with -1 for non-inliers)
// under the readings of DESIGN.md section 4 (the PnPsolver rows).  cvSVD is READ as OpenCV 2.4's Jacobi, not pinned (section 5).
//
// Three launches per call, none with atomics, each output written by one thread:
//   k_pnp_prepare      one workgroup per pair: the kept correspondences compacted in keypoint order by ballot prefix into 32-byte
//                      records (X, u, v, mvMaxError, the keypoint) in the scratch arena; N.
//   k_pnp_hypotheses   one wave per (pair, iteration of the window): the four indices from the caller's draws, EPnP with its
//                      matrices in LDS (pnp_epnp.h), then the lanes stride over the N records; the count is a sum of ballot popcounts.
//   k_pnp_select       one workgroup per pair: the stop rule over the window's counts; Refine runs where the best set changes
//                      (it is a pure function of that set), with the same EPnP shared out over the workgroup; every remaining output.
#include "kf_window.h"
#include "pnp_epnp.h"
#include <math.h>
#include <string>

#define PNP_T 256
#define PNP_WAVES (PNP_T / 64)
#define PNP_MAX_N 16000

struct PnpRec { float X[3], u, v, maxErr; int32_t kp, pad; };
static_assert(sizeof(PnpRec) == 32, "two dwordx4");
static_assert(sizeof(pgorb_pnp_hypothesis) == 104, "12 doubles and two int32");

struct PnpBatch {
    const pgorb_keypoint* K; const int32_t* n; int cap; const int32_t* pairFrame; const pgorb_kf_pose* cam;
    const int32_t* kpPoint; int npoints; const pgorb_map_point* pts; const uint8_t* pbad;
    int nlevels; float sigma2[PG_MAXL + 1];
    float th2; int first, niter, bestIn, wcap;
    const int32_t* dFirst; const int32_t* dBestIn; const uint32_t* draws; const int32_t* table;     // table[N] = {min inliers, cap}
    PnpRec* recs; int32_t* nKept; pgorb_pnp_hypothesis* hyps; double* work; uint8_t* maskBest; uint8_t* maskRef;
    uint8_t* bestInlier; pgorb_kf_pose* bestPose; pgorb_kf_pose* poseOut; uint8_t* inlier; int32_t* kpPointOut;
    pgorb_pnp_hypothesis* trace; int32_t* info; int32_t* nInl;
};

// exclusive prefix of `flag` over the workgroup in thread order, and the total
__device__ __forceinline__ void pnp_block_prefix(bool flag, int* cnt, int& before, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    before = 0; total = 0;
#pragma unroll
    for (int w = 0; w < PNP_WAVES; w++) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
    __syncthreads();
    before += __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(PNP_T) void k_pnp_prepare(PnpBatch B)
{
    __shared__ int cnt[PNP_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int f = B.pairFrame ? B.pairFrame[p] : p;
    const int nf = min(max(B.n[f], 0), B.cap);
    const int64_t row = (int64_t)p * B.cap;
    const pgorb_keypoint* K = B.K + (int64_t)f * B.cap;
    PnpRec* R = B.recs + row;
    int N = 0;
    for (int i0 = 0; i0 < B.cap; i0 += PNP_T) {
        const int i = i0 + tid;
        int s = i < nf ? B.kpPoint[row + i] : -1;
        if (s >= B.npoints) s = -1;
        if (s >= 0 && B.pbad && B.pbad[s]) s = -1;
        int o = 0;
        if (s >= 0) { o = K[i].octave; if (o < 0 || o >= B.nlevels) s = -1; }
        int before, total;
        pnp_block_prefix(s >= 0, cnt, before, total);
        if (s >= 0) {
            const pgorb_map_point A = B.pts[s];
            float4* dst = reinterpret_cast<float4*>(R + N + before);
            dst[0] = make_float4(A.pos[0], A.pos[1], A.pos[2], K[i].x);
            dst[1] = make_float4(K[i].y, __fmul_rn(B.sigma2[o], B.th2), __int_as_float(i), 0.0f);      // mvMaxError = mvSigma2*th2 (float)
        }
        N += total;
    }
    if (tid == 0) B.nKept[p] = N;
}

__device__ __forceinline__ PnpRec pnp_load(const PnpRec* r)
{
    const float4* s = reinterpret_cast<const float4*>(r);
    const float4 a = s[0], b = s[1];
    PnpRec R;
    R.X[0] = a.x; R.X[1] = a.y; R.X[2] = a.z; R.u = a.w; R.v = b.x; R.maxErr = b.y; R.kp = __float_as_int(b.z); R.pad = 0;
    return R;
}

__device__ __forceinline__ PnpCam pnp_cam(const PnpBatch& B, int p)
{
    const pgorb_kf_pose& P = B.cam[B.pairFrame ? B.pairFrame[p] : p];
    return PnpCam{(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy};
}

// CheckInliers (:308-339) for one correspondence: Xc, Yc, invZc are double expressions stored to float, ue / ve double,
// distX / distY float, error2 float against the float threshold; a NaN compares false
__device__ __forceinline__ bool pnp_inlier(const double* R, const double* t, const PnpCam& C, const PnpRec& r)
{
    const double X = (double)r.X[0], Y = (double)r.X[1], Z = (double)r.X[2];
    const float Xc = (float)(((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]);
    const float Yc = (float)(((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]);
    const float invZc = (float)(1.0 / (((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]));
    const double ue = C.uc + (C.fu * (double)Xc) * (double)invZc;
    const double ve = C.vc + (C.fv * (double)Yc) * (double)invZc;
    const float distX = (float)((double)r.u - ue), distY = (float)((double)r.v - ve);
    const float error2 = __fadd_rn(__fmul_rn(distX, distX), __fmul_rn(distY, distY));
    return error2 < r.maxErr;
}

// DUtils::Random::RandomInt(0, size - 1) of a raw rand() value
__device__ __forceinline__ int pnp_random_int(uint32_t r, int size)
{
    return (int)(((double)r / 2147483648.0) * (double)size);
}
// the indices iterate() takes from vAvailableIndices = 0 .. N-1 (the picked element is replaced by the back, the back is popped),
// without the list: only the positions a swap has overwritten are kept, every other position still holds its own index
template <int K> __device__ __forceinline__ void pnp_select(const uint32_t* d, int N, int* out)
{
    int pos[K], val[K];
    int size = N;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int r = pnp_random_int(d[j], size);
        int pick = r, back = size - 1;
#pragma unroll
        for (int a = 0; a < j; a++) { if (pos[a] == r) pick = val[a]; if (pos[a] == size - 1) back = val[a]; }    // the latest entry wins
        out[j] = pick;
        pos[j] = r; val[j] = back;
        size--;
    }
}

// the window of pair p: `w` iterations from `first`; empty when N < the adjusted min inliers
__device__ __forceinline__ void pnp_window(const PnpBatch& B, int p, int N, int& first, int& w, int& cap, int& minInl)
{
    first = max(B.dFirst ? B.dFirst[p] : B.first, 0);
    const int e = min(max(N, 0), B.cap);
    minInl = B.table[2 * e]; cap = B.table[2 * e + 1];
    w = N < minInl ? 0 : min(max(cap - first, B.niter), B.wcap);
}

__device__ __forceinline__ void pnp_put_hyp(pgorb_pnp_hypothesis* H, const double* R, const double* t, int inl, int flags)
{
#pragma unroll
    for (int k = 0; k < 9; k++) H->R[k] = R ? R[k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) H->t[k] = t ? t[k] : 0.0;
    H->inliers = inl; H->flags = flags;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(PnpBatch B)
{
    __shared__ PnpWork S;
    __shared__ double pt[4 * PNP_PT_DOUBLES];
    const int p = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const int N = B.nKept[p];
    int first, w, cap, minInl;
    pnp_window(B, p, N, first, w, cap, minInl);
    pgorb_pnp_hypothesis* H = B.hyps + (int64_t)p * B.wcap + k;
    pgorb_pnp_hypothesis* T = B.trace ? B.trace + (int64_t)p * B.wcap + k : nullptr;
    if (k >= w) {
        if (lane == 0) { pnp_put_hyp(H, nullptr, nullptr, 0, 0); if (T) pnp_put_hyp(T, nullptr, nullptr, 0, 0); }
        return;
    }
    const PnpRec* R = B.recs + (int64_t)p * B.cap;
    int idx[4];
    pnp_select<4>(B.draws + ((int64_t)p * B.wcap + k) * 4, N, idx);
    const PnpPts P = pnp_pts(pt, 4, 4);
    if (lane < 4) {
        const PnpRec r = pnp_load(R + min(max(idx[lane], 0), N - 1));      // (a draw >= 2^31 in the unchecked form)
        P.pws[3 * lane] = (double)r.X[0]; P.pws[3 * lane + 1] = (double)r.X[1]; P.pws[3 * lane + 2] = (double)r.X[2];
        P.us[2 * lane] = (double)r.u; P.us[2 * lane + 1] = (double)r.v;
    }
    const PnpCam C = pnp_cam(B, p);
    pnp_compute_pose(S, P, C, lane, 64);
    int inl = 0;
    for (int e0 = 0; e0 < N; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < N && pnp_inlier(S.Rb, S.tb, C, pnp_load(R + e));
        inl += __popcll(__ballot(in));
    }
    if (lane == 0) { pnp_put_hyp(H, S.Rb, S.tb, inl, 1); if (T) pnp_put_hyp(T, S.Rb, S.tb, inl, 1); }
}

// a complete pgorb_kf_pose from a float [R | t]: Frame::SetPose's mOw = -Rcw.t()*tcw as pose_opt.hip reads it, the camera copied
__device__ __forceinline__ void pnp_put_pose(pgorb_kf_pose* o, const pgorb_kf_pose& cam, const float* R, const float* t)
{
    pgorb_kf_pose q = cam;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) q.Tcw[4 * r + c] = R[3 * r + c];
        q.Tcw[4 * r + 3] = t[r];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        q.Ow[i] = cnm_f(__dmul_rn((double)cnm_dot3f(q.Tcw[i], q.Tcw[4 + i], q.Tcw[8 + i], q.Tcw[3], q.Tcw[7], q.Tcw[11]), -1.0));
    *o = q;
}

// mask[e] = CheckInliers' flag of record e under (R, t); the count
__device__ __forceinline__ int pnp_mask(const double* R, const double* t, const PnpCam& C, const PnpRec* rec, int N, uint8_t* mask)
{
    int cnt = 0;
    for (int e0 = 0; e0 < N; e0 += PNP_T) {
        const int e = e0 + (int)threadIdx.x;
        const bool in = e < N && pnp_inlier(R, t, C, pnp_load(rec + e));
        if (e < N) mask[e] = in ? 1 : 0;
        cnt += __syncthreads_count(in);
    }
    return cnt;
}

__global__ __launch_bounds__(PNP_T) void k_pnp_select(PnpBatch B)
{
    __shared__ PnpWork S;
    __shared__ int cnt[PNP_WAVES];
    __shared__ double hyp[12];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int N = B.nKept[p];
    int first, w, cap, minInl;
    pnp_window(B, p, N, first, w, cap, minInl);
    const int64_t row = (int64_t)p * B.cap;
    const int f = B.pairFrame ? B.pairFrame[p] : p;
    const PnpRec* rec = B.recs + row;
    const pgorb_pnp_hypothesis* H = B.hyps + (int64_t)p * B.wcap;
    uint8_t* maskBest = B.maskBest + row;
    uint8_t* maskRef = B.maskRef + row;
    const PnpCam C = pnp_cam(B, p);
    const pgorb_kf_pose camPose = B.cam[f];
    int best = B.dBestIn ? B.dBestIn[p] : B.bestIn;
    if (!B.bestInlier || !B.bestPose) best = 0;                         // a count without its set and pose carries nothing
    // the state carried in: mvbBestInliers by keypoint -> by record; mBestTcw
    for (int e = tid; e < N; e += PNP_T) maskBest[e] = B.bestInlier ? B.bestInlier[row + pnp_load(rec + e).kp] : 0;
    float bestR[9], bestT[3];
    bool havePose = false;
    if (B.bestPose && best > 0) {
        const pgorb_kf_pose q = B.bestPose[p];
#pragma unroll
        for (int r = 0; r < 3; r++) { bestR[3 * r] = q.Tcw[4 * r]; bestR[3 * r + 1] = q.Tcw[4 * r + 1]; bestR[3 * r + 2] = q.Tcw[4 * r + 2]; bestT[r] = q.Tcw[4 * r + 3]; }
        havePose = true;
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) bestR[k] = 0.0f;
        bestT[0] = bestT[1] = bestT[2] = 0.0f;
    }
    __syncthreads();

    int its = first, foundK = -1, refCount = 0, status = 0;
    bool known = false;                 // Refine's result on the current best set is in maskRef / S.Rb / refCount
    float refR[9], refT[3];
    for (int k = 0; k < w; k++) {
        its = first + k + 1;
        const int c = H[k].inliers;
        if (c < minInl) continue;
        if (c > best) {                                                 // strictly better: mvbBestInliers, mnBestInliers, mBestTcw
            best = c;
            if (tid < 12) hyp[tid] = tid < 9 ? H[k].R[tid] : H[k].t[tid - 9];
            __syncthreads();
            pnp_mask(hyp, hyp + 9, C, rec, N, maskBest);
#pragma unroll
            for (int q = 0; q < 9; q++) bestR[q] = (float)hyp[q];
#pragma unroll
            for (int q = 0; q < 3; q++) bestT[q] = (float)hyp[9 + q];
            havePose = true;
            known = false;
            __syncthreads();
        }
        if (!known) {
            // Refine (:260-305): the best set's correspondences in order, compute_pose, CheckInliers
            double* base = B.work + (int64_t)p * B.cap * PNP_PT_DOUBLES;
            int n = 0;
            for (int e0 = 0; e0 < N; e0 += PNP_T) {
                const int e = e0 + tid;
                const bool on = e < N && maskBest[e];
                int before, total;
                pnp_block_prefix(on, cnt, before, total);
                if (on) {
                    const PnpRec r = pnp_load(rec + e);
                    const int d = n + before;
                    double* pw = base + 3 * (int64_t)d;
                    double* us = base + 3 * (int64_t)B.cap + 2 * (int64_t)d;
                    pw[0] = (double)r.X[0]; pw[1] = (double)r.X[1]; pw[2] = (double)r.X[2];
                    us[0] = (double)r.u; us[1] = (double)r.v;
                }
                n += total;
            }
            const PnpPts P = pnp_pts(base, n, B.cap);
            pnp_compute_pose(S, P, C, tid, PNP_T);
            refCount = pnp_mask(S.Rb, S.tb, C, rec, N, maskRef);
#pragma unroll
            for (int q = 0; q < 9; q++) refR[q] = (float)S.Rb[q];
#pragma unroll
            for (int q = 0; q < 3; q++) refT[q] = (float)S.tb[q];
            known = true;
            __syncthreads();
        }
        if (refCount > minInl) { foundK = k; break; }
    }

    int nInl = 0;
    const uint8_t* outMask = nullptr;
    const float* oR = nullptr; const float* oT = nullptr;
    if (N < minInl) status = PGORB_PNP_FEW | PGORB_PNP_NO_MORE;
    else if (foundK >= 0) { status = PGORB_PNP_FOUND | PGORB_PNP_REFINED; nInl = refCount; outMask = maskRef; oR = refR; oT = refT; }
    else if (its >= cap) {
        status = PGORB_PNP_NO_MORE;
        if (best >= minInl && havePose) { status |= PGORB_PNP_FOUND; nInl = best; outMask = maskBest; oR = bestR; oT = bestT; }
    }
    // every per-keypoint output cleared, then the flags by keypoint (Tracking.cc:1405-1420: a non-inlier's point is NULL)
    const bool writeBest = B.bestInlier && !(status & PGORB_PNP_FEW);
    for (int i = tid; i < B.cap; i += PNP_T) {
        B.inlier[row + i] = 0;
        B.kpPointOut[row + i] = -1;
        if (writeBest) B.bestInlier[row + i] = 0;
    }
    __syncthreads();
    for (int e = tid; e < N; e += PNP_T) {
        const int kp = pnp_load(rec + e).kp;
        if (outMask && outMask[e]) { B.inlier[row + kp] = 1; B.kpPointOut[row + kp] = B.kpPoint[row + kp]; }
        if (writeBest && maskBest[e]) B.bestInlier[row + kp] = 1;
    }
    if (tid == 0) {
        if (oR) pnp_put_pose(B.poseOut + p, camPose, oR, oT);
        else { pgorb_kf_pose z; memset(&z, 0, sizeof(z)); B.poseOut[p] = z; }
        if (B.bestPose && !(status & PGORB_PNP_FEW)) {
            if (havePose) pnp_put_pose(B.bestPose + p, camPose, bestR, bestT);
            else { pgorb_kf_pose z; memset(&z, 0, sizeof(z)); B.bestPose[p] = z; }
        }
        if (B.nInl) B.nInl[p] = nInl;
        if (B.info) {
            int32_t* I = B.info + (int64_t)p * PGORB_PNP_INFO;
            I[0] = status; I[1] = N; I[2] = minInl; I[3] = cap; I[4] = (status & PGORB_PNP_FEW) ? first : its; I[5] = nInl; I[6] = best;
            I[7] = foundK >= 0 ? first + foundK : -1;
        }
    }
}

static const char* pnp_params_why(const pgorb_pnp_params* P)
{
    if (!P) return "params is NULL";
    if (P->min_set != 4) return "min_set is not 4";
    if (P->min_inliers < 1) return "min_inliers is below 1";
    if (!(P->probability > 0.0f && P->probability < 1.0f)) return "probability is outside (0, 1)";
    if (!(P->epsilon > 0.0f && P->epsilon <= 1.0f)) return "epsilon is outside (0, 1]";
    if (!(P->th2 > 0.0f)) return "th2 is not positive";
    if (P->max_iterations < 1) return "max_iterations is below 1";
    if (P->first_iteration < 0) return "first_iteration is negative";
    if (P->niterations < 1) return "niterations is below 1";
    if (P->best_inliers_in < 0) return "best_inliers_in is negative";
    return nullptr;
}

static int pnp_window_cap(const pgorb_pnp_params* P) { return std::max(P->max_iterations, P->niterations); }

extern "C" {

int pgorb_pnp_ransac(float probability, int min_inliers, int max_iterations, int min_set, float epsilon, int N,
                     int32_t* min_inliers_out, int32_t* max_iterations_out)
{
    int32_t a, b;
    pg_pnp_ransac(probability, min_inliers, max_iterations, min_set, epsilon, N, &a, &b);
    if (min_inliers_out) *min_inliers_out = a;
    if (max_iterations_out) *max_iterations_out = b;
    return 0;
}

int pgorb_pnp_solver_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap, const int32_t* d_pair_frame,
        int npairs, const pgorb_kf_pose* d_camera, const int32_t* d_kp_point, int npoints, const pgorb_map_point* d_points,
        const uint8_t* d_point_bad, const pgorb_pnp_params* params, const int32_t* d_first_iteration, const int32_t* d_best_inliers_in,
        const uint32_t* d_draws, uint8_t* d_best_inlier, pgorb_kf_pose* d_best_pose, pgorb_kf_pose* d_pose_out, uint8_t* d_inlier,
        int32_t* d_kp_point_out, pgorb_pnp_hypothesis* d_trace, int32_t* d_info, int32_t* d_ninliers, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || cap < 1 || npairs < 0 || npoints < 0 ||
        (npairs && (!d_camera || !d_kp_point || !d_draws || !d_pose_out || !d_inlier || !d_kp_point_out)) || (npoints && !d_points))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_pnp_solver_batch_device");
    if (const char* why = pnp_params_why(params)) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_pnp_solver: ") + why).c_str());
    if (cap > PNP_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pnp_solver: more than 16000 keypoints per frame");
    if (pnp_window_cap(params) > PGORB_PNP_MAX_WINDOW) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pnp_solver: a window above PGORB_PNP_MAX_WINDOW");
    if (!npairs) return 0;
    PnpBatch B;
    B.nlevels = pgorb_levels(c);
    memset(B.sigma2, 0, sizeof(B.sigma2));
    if (!(B.nlevels > 0) || B.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, B.sigma2, nullptr) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    hipStream_t s = (hipStream_t)stream;
    int rc = pg_ctx_pnp_table(c, params->probability, params->min_inliers, params->max_iterations, params->min_set, params->epsilon, PNP_MAX_N, &B.table);
    if (rc) return rc;
    B.wcap = pnp_window_cap(params);
    PgCarve L;
    const size_t oRec = L.take((size_t)npairs * cap * sizeof(PnpRec)), oHyp = L.take((size_t)npairs * B.wcap * sizeof(pgorb_pnp_hypothesis)),
                 oWork = L.take((size_t)npairs * cap * PNP_PT_DOUBLES * 8), oMB = L.take((size_t)npairs * cap), oMR = L.take((size_t)npairs * cap),
                 oN = L.take((size_t)npairs * 4);
    void* scr;
    if ((rc = pg_ctx_scratch(c, L.o, s, &scr))) return rc;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.pairFrame = d_pair_frame; B.cam = d_camera; B.kpPoint = d_kp_point;
    B.npoints = npoints; B.pts = d_points; B.pbad = d_point_bad;
    B.th2 = params->th2; B.first = params->first_iteration; B.niter = params->niterations; B.bestIn = params->best_inliers_in;
    B.dFirst = d_first_iteration; B.dBestIn = d_best_inliers_in; B.draws = d_draws;
    uint8_t* base = (uint8_t*)scr;
    B.recs = (PnpRec*)(base + oRec); B.hyps = (pgorb_pnp_hypothesis*)(base + oHyp); B.work = (double*)(base + oWork);
    B.maskBest = base + oMB; B.maskRef = base + oMR; B.nKept = (int32_t*)(base + oN);
    B.bestInlier = d_best_inlier; B.bestPose = d_best_pose; B.poseOut = d_pose_out; B.inlier = d_inlier; B.kpPointOut = d_kp_point_out;
    B.trace = d_trace; B.info = d_info; B.nInl = d_ninliers;
    hipLaunchKernelGGL(k_pnp_prepare, dim3((unsigned)npairs), dim3(PNP_T), 0, s, B);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)B.wcap, (unsigned)npairs), dim3(64), 0, s, B);
    hipLaunchKernelGGL(k_pnp_select, dim3((unsigned)npairs), dim3(PNP_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "a PnPsolver kernel launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool pnp_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

int pgorb_pnp_solver(pgorb_ctx* c, const pgorb_keypoint* kps, int n, const pgorb_kf_pose* camera, const int32_t* kp_point, int npoints,
        const pgorb_map_point* points, const uint8_t* point_bad, const pgorb_pnp_params* params, const uint32_t* draws,
        const uint8_t* best_inlier_in, const pgorb_kf_pose* best_pose_in, pgorb_kf_pose* pose_out, uint8_t* inlier, int32_t* kp_point_out,
        uint8_t* best_inlier_out, pgorb_kf_pose* best_pose_out, pgorb_pnp_hypothesis* trace, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    if (n < 0 || npoints < 0) why = "a count is negative";
    else if (!camera || !params || !draws || !pose_out || (n && (!kps || !kp_point || !inlier || !kp_point_out)) || (npoints && !points))
        why = "an array that is read or written is NULL";
    else why = pnp_params_why(params);
    if (!why && !pnp_all_finite(&camera->fx, 4)) why = "the camera is not finite";
    if (!why && best_pose_in && !pnp_all_finite(best_pose_in->Tcw, 12)) why = "best_pose_in is not finite";
    for (int i = 0; !why && i < n; i++) {
        const int s = kp_point[i];
        if (s < -1 || s >= npoints) { why = "a slot's point index is out of range"; break; }
        if (s < 0 || (point_bad && point_bad[s])) continue;
        if (kps[i].octave < 0 || kps[i].octave >= nlevels) why = "an octave is outside the context's levels";
        else if (!pnp_all_finite(points[s].pos, 3) || !pnp_all_finite(&kps[i].x, 2)) why = "a referenced point or keypoint is not finite";
    }
    const int wcap = why ? 0 : pnp_window_cap(params);
    if (!why && wcap <= PGORB_PNP_MAX_WINDOW)
        for (int64_t k = 0; k < (int64_t)wcap * 4; k++)
            if (draws[k] >= 0x80000000u) { why = "a draw is not below 2^31"; break; }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_pnp_solver: ") + why).c_str());
    if (n > PNP_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pnp_solver: more than 16000 keypoints per frame");
    if (wcap > PGORB_PNP_MAX_WINDOW) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_pnp_solver: a window above PGORB_PNP_MAX_WINDOW");
    const int cap = std::max(n, 1), np = std::max(npoints, 1);
    const size_t nd = (size_t)wcap * 16, nt = trace ? (size_t)wcap * sizeof(pgorb_pnp_hypothesis) : 0;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)cap * sizeof(pgorb_keypoint)), oCam = s.region(PG_UP, sizeof(pgorb_kf_pose)),
                 oS = s.region(PG_UP, (size_t)cap * 4), oP = s.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)),
                 oB = s.region(PG_UP, point_bad ? np : 0), oD = s.region(PG_UP, nd),
                 oBI = s.region(PG_INOUT, cap), oBP = s.region(PG_INOUT, sizeof(pgorb_kf_pose)),
                 oPose = s.region(PG_DOWN, sizeof(pgorb_kf_pose)), oI = s.region(PG_DOWN, cap), oKO = s.region(PG_DOWN, (size_t)cap * 4),
                 oT = s.region(PG_DOWN, nt), oR = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t cnt[4] = {n, 0, 0, 0};
    s.put(oN, cnt, 16);
    s.put(oK, kps, (size_t)n * sizeof(pgorb_keypoint), 0, (size_t)cap * sizeof(pgorb_keypoint));
    s.put(oCam, camera, sizeof(pgorb_kf_pose));
    memset(s.host(oS), 0xFF, (size_t)cap * 4);
    s.put(oS, kp_point, (size_t)n * 4);
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    if (point_bad) s.put(oB, point_bad, npoints, 0, np);
    s.put(oD, draws, nd);
    s.put(oBI, best_inlier_in, n, 0, cap);
    s.put(oBP, best_pose_in, sizeof(pgorb_kf_pose), 0, sizeof(pgorb_kf_pose));
    pgorb_pnp_params P = *params;
    if (!best_pose_in || !best_inlier_in) P.best_inliers_in = 0;        // a count without its set and pose carries nothing
    int32_t* R = s.dev<int32_t>(oR);                                    // ninliers, -, info[8] from R + 2
    if ((rc = s.run([&] {
            return pgorb_pnp_solver_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), cap, nullptr, 1, s.dev<pgorb_kf_pose>(oCam),
                                                 s.dev<int32_t>(oS), npoints, s.dev<pgorb_map_point>(oP), point_bad ? s.dev(oB) : nullptr, &P,
                                                 nullptr, nullptr, s.dev<uint32_t>(oD), s.dev(oBI), s.dev<pgorb_kf_pose>(oBP),
                                                 s.dev<pgorb_kf_pose>(oPose), s.dev(oI), s.dev<int32_t>(oKO),
                                                 trace ? s.dev<pgorb_pnp_hypothesis>(oT) : nullptr, R + 2, R, nullptr); }))) return rc;
    memcpy(pose_out, s.host(oPose), sizeof(pgorb_kf_pose));
    if (n) { memcpy(inlier, s.host(oI), n); memcpy(kp_point_out, s.host(oKO), (size_t)n * 4); }
    if (best_inlier_out && n) memcpy(best_inlier_out, s.host(oBI), n);
    if (best_pose_out) memcpy(best_pose_out, s.host(oBP), sizeof(pgorb_kf_pose));
    if (trace) memcpy(trace, s.host(oT), nt);
    const int32_t* r = s.host<int32_t>(oR);
    if (info) memcpy(info, r + 2, PGORB_PNP_INFO * 4);
    return r[0];
}

}  // extern "C"
