// sim3.hip -- Sim3Solver on gfx950: the RANSAC Horn alignment of a loop candidate's matches, every hypothesis of the requested
// window evaluated at once and the reference's sequential stop rule applied afterwards as a prefix-max scan.
//
// Restates (thirdparty/orb-slam2):
//   Sim3Solver::Sim3Solver                        src/Sim3Solver.cc:37-112 (the correspondences, in i1 order; mvnMaxError1/2 are size_t)
//   Sim3Solver::SetRansacParameters               :114-138 (on the host: pg_sim3_cap, api.hip)
//   Sim3Solver::iterate / find                    :140-213
//   Sim3Solver::ComputeCentroid / ComputeSim3     :215-337 (Horn 1987)
//   Sim3Solver::CheckInliers / Project / FromCameraToImage   :340-423
//   DUtils::Random::RandomInt                     DUtils/Random.cpp:47-50
//   LoopClosing::ComputeSim3                      src/LoopClosing.cc:313-318 (matches12_out), ORBmatcher.cc:1133-1146 (already1 / 2)
// under the cv::Mat readings of DESIGN.md section 4 (the Sim3Solver rows).  cv::eigen is READ as a cyclic Jacobi in double on the float
// N, not pinned: OpenCV 2.4.9 cannot be built here.
//
// Three launches per call, none with atomics, each output written by one lane:
//   k_sim3_prepare     one workgroup per pair: the kept correspondences compacted in i1 order by ballot prefix into 64-byte records
//                      (X3Dc1, X3Dc2, their images, the two truncated thresholds, i1, i2) in the scratch arena; N; every per-keypoint
//                      output cleared.
//   k_sim3_hypotheses  one wave per (pair, iteration of the window): the triple from the caller's draws, Horn computed identically by
//                      every lane, then the lanes stride over the N records; the count is a sum of ballot popcounts.
//   k_sim3_select      one wave per pair: the stop rule over the window's counts, the flags of the returned hypothesis recomputed by
//                      the same function, every remaining output.
#include "kf_window.h"
#include <math.h>
#include <string>

#define S3_T 256
#define S3_WAVES (S3_T / 64)
#define S3_MAX_N 16000

struct S3Rec { float X1[3], X2[3], p1[2], p2[2], th1, th2; int32_t i1, i2; float pad[2]; };
static_assert(sizeof(S3Rec) == 64, "four dwordx4");
struct S3Hyp { float R[9], t[3], s; int32_t inl; float pad[2]; };
static_assert(sizeof(S3Hyp) == 64, "four dwordx4");

struct S3Batch {
    const pgorb_keypoint* K; const int32_t* n; int cap; const int32_t* pairKF1; const int32_t* pairKF2; const pgorb_kf_pose* pose;
    const int32_t* kfPoint; const int32_t* matches12; int npoints; const pgorb_map_point* pts; const uint8_t* pbad;
    int nlevels; float sigma2[PG_MAXL + 1];
    int minInliers, fixScale, first, niter, bestIn, maxIts;
    const int32_t* dFirst; const int32_t* dBestIn; const uint32_t* draws; const int32_t* caps;
    S3Rec* recs; int32_t* nKept; S3Hyp* hyps;
    pgorb_sim3_estimate* found; pgorb_sim3* foundSim3; pgorb_sim3_estimate* best; uint8_t* inlier; int32_t* matchesOut;
    uint8_t* already1; uint8_t* already2; int32_t* info; int32_t* nInl;
};

// FromCameraToImage / Project's tail: invz = 1/z, x*invz, fx*x + cx in float
__device__ __forceinline__ void s3_image(const float* X, float fx, float fy, float cx, float cy, float& u, float& v)
{
    const float invz = __fdiv_rn(1.0f, X[2]);
    u = __fadd_rn(__fmul_rn(fx, __fmul_rn(X[0], invz)), cx);
    v = __fadd_rn(__fmul_rn(fy, __fmul_rn(X[1], invz)), cy);
}

__global__ __launch_bounds__(S3_T) void k_sim3_prepare(S3Batch B)
{
    __shared__ int cnt[S3_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f1 = B.pairKF1 ? B.pairKF1[p] : 0, f2 = B.pairKF2 ? B.pairKF2[p] : 1;
    const int n1 = min(max(B.n[f1], 0), B.cap), n2 = min(max(B.n[f2], 0), B.cap);
    const int64_t row = (int64_t)p * B.cap;
    const pgorb_keypoint* K1 = B.K + (int64_t)f1 * B.cap;
    const pgorb_keypoint* K2 = B.K + (int64_t)f2 * B.cap;
    const int32_t* S1 = B.kfPoint + (int64_t)f1 * B.cap;
    const int32_t* S2 = B.kfPoint + (int64_t)f2 * B.cap;
    const pgorb_kf_pose P1 = B.pose[f1], P2 = B.pose[f2];
    S3Rec* R = B.recs + row;
    int N = 0;
    for (int i0 = 0; i0 < B.cap; i0 += S3_T) {
        const int i1 = i0 + tid;
        int i2 = i1 < n1 ? B.matches12[row + i1] : -1;
        if (i2 < 0 || i2 >= n2) i2 = -1;
        int s1 = -1, s2 = -1, o1 = 0, o2 = 0;
        if (i2 >= 0) {
            s1 = S1[i1]; s2 = S2[i2];
            if (s1 < 0 || s1 >= B.npoints || s2 < 0 || s2 >= B.npoints) i2 = -1;
        }
        if (i2 >= 0 && B.pbad && (B.pbad[s1] | B.pbad[s2])) i2 = -1;
        if (i2 >= 0) {
            o1 = K1[i1].octave; o2 = K2[i2].octave;
            if (o1 < 0 || o1 >= B.nlevels || o2 < 0 || o2 >= B.nlevels) i2 = -1;
        }
        const unsigned long long m = __ballot(i2 >= 0);
        if (lane == 0) cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < S3_WAVES; w++) { const int c = cnt[w]; if (w < wave) before += c; total += c; }
        __syncthreads();
        if (i2 >= 0) {
            const int e = N + before + __popcll(m & ((1ull << lane) - 1ull));
            const pgorb_map_point A = B.pts[s1], C = B.pts[s2];
            float X1[3], X2[3], u1, v1, u2, v2;
            kf_to_camera(P1, A.pos, X1);
            kf_to_camera(P2, C.pos, X2);
            s3_image(X1, P1.fx, P1.fy, P1.cx, P1.cy, u1, v1);
            s3_image(X2, P2.fx, P2.fy, P2.cx, P2.cy, u2, v2);
            // mvnMaxError: 9.210*sigma2 in double, truncated to size_t, compared as float
            const float th1 = (float)(unsigned long long)__dmul_rn(9.210, (double)B.sigma2[o1]);
            const float th2 = (float)(unsigned long long)__dmul_rn(9.210, (double)B.sigma2[o2]);
            float4* dst = reinterpret_cast<float4*>(R + e);
            dst[0] = make_float4(X1[0], X1[1], X1[2], X2[0]);
            dst[1] = make_float4(X2[1], X2[2], u1, v1);
            dst[2] = make_float4(u2, v2, th1, th2);
            dst[3] = make_float4(__int_as_float(i1), __int_as_float(i2), 0.0f, 0.0f);
        }
        if (i1 < B.cap) {
            B.inlier[row + i1] = 0;
            B.matchesOut[row + i1] = -1;
            if (B.already1) B.already1[row + i1] = 0;
            if (B.already2) B.already2[row + i1] = 0;
        }
        N += total;
    }
    if (tid == 0) B.nKept[p] = N;
}

__device__ __forceinline__ S3Rec s3_load(const S3Rec* r)
{
    const float4* s = reinterpret_cast<const float4*>(r);
    const float4 a = s[0], b = s[1], c = s[2], d = s[3];
    S3Rec R;
    R.X1[0] = a.x; R.X1[1] = a.y; R.X1[2] = a.z; R.X2[0] = a.w; R.X2[1] = b.x; R.X2[2] = b.y;
    R.p1[0] = b.z; R.p1[1] = b.w; R.p2[0] = c.x; R.p2[1] = c.y; R.th1 = c.z; R.th2 = c.w;
    R.i1 = __float_as_int(d.x); R.i2 = __float_as_int(d.y); R.pad[0] = 0.0f; R.pad[1] = 0.0f;
    return R;
}

// DUtils::Random::RandomInt(0, size - 1) of a raw rand() value
__device__ __forceinline__ int s3_random_int(uint32_t r, int size)
{
    return (int)(((double)r / 2147483648.0) * (double)size);
}
// the three indices iterate() takes from vAvailableIndices = 0 .. N-1: the picked element is replaced by the back, the back is popped.
// After the first pick position r0 holds N-1; after the second, position r1 holds what position N-2 held.
__device__ __forceinline__ void s3_triple(const uint32_t* d, int N, int& a, int& b, int& c)
{
    const int r0 = s3_random_int(d[0], N), r1 = s3_random_int(d[1], N - 1), r2 = s3_random_int(d[2], N - 2);
    a = r0;
    b = r1 == r0 ? N - 1 : r1;
    const int moved = (N - 2) == r0 ? N - 1 : N - 2;
    c = r2 == r1 ? moved : (r2 == r0 ? N - 1 : r2);
}

// One rotation of the cyclic Jacobi on the symmetric A (both triangles kept) with the eigenvectors as V's columns
#define S3_ROT(P, Q) do { \
        const double apq = A[P][Q]; \
        if (apq != 0.0) { \
            const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq); \
            const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __dsqrt_rn(theta * theta + 1.0)); \
            const double cc = 1.0 / __dsqrt_rn(tt * tt + 1.0), ss = tt * cc; \
            _Pragma("unroll") for (int k = 0; k < 4; k++) { \
                const double akp = A[k][P], akq = A[k][Q]; \
                A[k][P] = cc * akp - ss * akq; A[k][Q] = ss * akp + cc * akq; } \
            _Pragma("unroll") for (int k = 0; k < 4; k++) { \
                const double apk = A[P][k], aqk = A[Q][k]; \
                A[P][k] = cc * apk - ss * aqk; A[Q][k] = ss * apk + cc * aqk; } \
            _Pragma("unroll") for (int k = 0; k < 4; k++) { \
                const double vkp = V[k][P], vkq = V[k][Q]; \
                V[k][P] = cc * vkp - ss * vkq; V[k][Q] = ss * vkp + cc * vkq; } \
            A[P][Q] = 0.0; A[Q][P] = 0.0; \
        } } while (0)

struct S3Sim { float R[9], t[3], s, sR12[9], sR21[9], t21[3]; };

// ComputeSim3 (:226-337) on the three correspondences a, b, c (the columns of P3Dc1i / P3Dc2i)
__device__ __forceinline__ void s3_horn(const S3Rec& a, const S3Rec& b, const S3Rec& c, int fixScale, S3Sim& T)
{
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];                       // [row][column]
    const float third = cnm_f(1.0 / 3.0);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        // cv::reduce(SUM) along the row: (p0 + p2) + p1; C/P.cols: the scaled copy by (float)(1.0/3)
        O1[r] = __fmul_rn(__fadd_rn(__fadd_rn(a.X1[r], c.X1[r]), b.X1[r]), third);
        O2[r] = __fmul_rn(__fadd_rn(__fadd_rn(a.X2[r], c.X2[r]), b.X2[r]), third);
        Pr1[r][0] = __fsub_rn(a.X1[r], O1[r]); Pr1[r][1] = __fsub_rn(b.X1[r], O1[r]); Pr1[r][2] = __fsub_rn(c.X1[r], O1[r]);
        Pr2[r][0] = __fsub_rn(a.X2[r], O2[r]); Pr2[r][1] = __fsub_rn(b.X2[r], O2[r]); Pr2[r][2] = __fsub_rn(c.X2[r], O2[r]);
    }
    // M = Pr2*Pr1.t(): a transposed operand, sums in double from 0, rounded once
    float M[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) M[r][q] = cnm_f(cnm_dotd(Pr2[r][0], Pr2[r][1], Pr2[r][2], Pr1[q][0], Pr1[q][1], Pr1[q][2]));
    // N: float expressions left to right, widened to double and stored as float again (exact)
    const float N11 = __fadd_rn(__fadd_rn(M[0][0], M[1][1]), M[2][2]), N12 = __fsub_rn(M[1][2], M[2][1]), N13 = __fsub_rn(M[2][0], M[0][2]),
                N14 = __fsub_rn(M[0][1], M[1][0]), N22 = __fsub_rn(__fsub_rn(M[0][0], M[1][1]), M[2][2]), N23 = __fadd_rn(M[0][1], M[1][0]),
                N24 = __fadd_rn(M[2][0], M[0][2]), N33 = __fsub_rn(__fadd_rn(-M[0][0], M[1][1]), M[2][2]), N34 = __fadd_rn(M[1][2], M[2][1]),
                N44 = __fadd_rn(__fsub_rn(-M[0][0], M[1][1]), M[2][2]);
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    // cv::eigen, READ as: cyclic Jacobi in double, swept until the off-diagonal part has vanished against the diagonal (at most 32 sweeps)
    for (int sweep = 0; sweep < 32; sweep++) {
        const double off = ((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + (A[0][3] * A[0][3] + A[1][2] * A[1][2])) + (A[1][3] * A[1][3] + A[2][3] * A[2][3]);
        const double dg = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + (A[2][2] * A[2][2] + A[3][3] * A[3][3]);
        if (!(off > 1e-36 * dg)) break;
        S3_ROT(0, 1); S3_ROT(0, 2); S3_ROT(0, 3); S3_ROT(1, 2); S3_ROT(1, 3); S3_ROT(2, 3);
    }
    // row 0 of evec: the eigenvector of the largest eigenvalue (the first of equal ones), as float
    int kb = 0;
    double eb = A[0][0];
    if (A[1][1] > eb) { eb = A[1][1]; kb = 1; }
    if (A[2][2] > eb) { eb = A[2][2]; kb = 2; }
    if (A[3][3] > eb) { eb = A[3][3]; kb = 3; }
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = cnm_f(kb == 0 ? V[k][0] : kb == 1 ? V[k][1] : kb == 2 ? V[k][2] : V[k][3]);
    // ang = atan2(norm(vec), w); vec = 2*ang*vec/norm(vec): one scaled copy by (float)((2*ang)*(1/norm))
    const double nrm = cnm_normd(q[1], q[2], q[3]);
    const double ang = atan2(nrm, (double)q[0]);
    const float sc = cnm_f((2.0 * ang) * (1.0 / nrm));
    const float rv[3] = {__fmul_rn(q[1], sc), __fmul_rn(q[2], sc), __fmul_rn(q[3], sc)};
    // cv::Rodrigues (vector -> matrix) in double, narrowed to float
    {
        double rx = rv[0], ry = rv[1], rz = rv[2];
        const double theta = __dsqrt_rn((rx * rx + ry * ry) + rz * rz);
        if (theta < 2.220446049250313e-16) {
#pragma unroll
            for (int k = 0; k < 9; k++) T.R[k] = k % 4 == 0 ? 1.0f : 0.0f;
        } else {
            const double co = cos(theta), si = sin(theta), c1 = 1.0 - co, it = theta != 0.0 ? 1.0 / theta : 0.0;
            rx *= it; ry *= it; rz *= it;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double rxm[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
#pragma unroll
            for (int k = 0; k < 9; k++) T.R[k] = cnm_f((co * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + si * rxm[k]);
        }
    }
    // P3 = R*Pr2 (gemm's small-matrix path); nom = Pr1.dot(P3) and den = the sum of cv::pow(P3, 2)'s float squares, in double, row-major
    if (!fixScale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float p3 = cnm_dot3f(T.R[3 * r], T.R[3 * r + 1], T.R[3 * r + 2], Pr2[0][k], Pr2[1][k], Pr2[2][k]);
                nom = __dadd_rn(nom, __dmul_rn((double)Pr1[r][k], (double)p3));
                den = __dadd_rn(den, (double)__fmul_rn(p3, p3));
            }
        T.s = cnm_f(nom / den);
    } else T.s = 1.0f;
    // t12 = O1 - s*R*O2: the product on gemm's small-matrix path with alpha = s in double, then a float subtraction
    const double sd = (double)T.s;
#pragma unroll
    for (int r = 0; r < 3; r++)
        T.t[r] = __fsub_rn(O1[r], cnm_f(__dmul_rn((double)cnm_dot3f(T.R[3 * r], T.R[3 * r + 1], T.R[3 * r + 2], O2[0], O2[1], O2[2]), sd)));
    // sR = s*R and sRinv = (1.0/s)*R.t(): scaled copies, the factor formed in double and applied in float; tinv = -sRinv*t12 (alpha = -1)
    const float si = cnm_f(1.0 / sd);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) { T.sR12[3 * r + k] = __fmul_rn(T.R[3 * r + k], T.s); T.sR21[3 * r + k] = __fmul_rn(T.R[3 * k + r], si); }
#pragma unroll
    for (int r = 0; r < 3; r++)
        T.t21[r] = cnm_f(__dmul_rn((double)cnm_dot3f(T.sR21[3 * r], T.sR21[3 * r + 1], T.sR21[3 * r + 2], T.t[0], T.t[1], T.t[2]), -1.0));
}

// the derived parts of a stored hypothesis (R, t, s), exactly as s3_horn forms them
__device__ __forceinline__ void s3_derive(S3Sim& T)
{
    const double sd = (double)T.s;
    const float si = cnm_f(1.0 / sd);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) { T.sR12[3 * r + k] = __fmul_rn(T.R[3 * r + k], T.s); T.sR21[3 * r + k] = __fmul_rn(T.R[3 * k + r], si); }
#pragma unroll
    for (int r = 0; r < 3; r++)
        T.t21[r] = cnm_f(__dmul_rn((double)cnm_dot3f(T.sR21[3 * r], T.sR21[3 * r + 1], T.sR21[3 * r + 2], T.t[0], T.t[1], T.t[2]), -1.0));
}

struct S3Cam { float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };

// CheckInliers for one correspondence: KF2's point into KF1 under T12 and K1, KF1's into KF2 under T21 and K2; err = dist.dot(dist)
// (a double sum rounded to float); a NaN compares false
__device__ __forceinline__ bool s3_inlier(const S3Sim& T, const S3Cam& C, const S3Rec& r)
{
    float Y[3], u, v;
#pragma unroll
    for (int k = 0; k < 3; k++) Y[k] = kf_row(T.sR12 + 3 * k, T.t[k], r.X2);
    s3_image(Y, C.fx1, C.fy1, C.cx1, C.cy1, u, v);
    const float d0 = __fsub_rn(r.p1[0], u), d1 = __fsub_rn(r.p1[1], v);
    const float err1 = cnm_f(__dadd_rn(__dadd_rn(0.0, __dmul_rn((double)d0, (double)d0)), __dmul_rn((double)d1, (double)d1)));
#pragma unroll
    for (int k = 0; k < 3; k++) Y[k] = kf_row(T.sR21 + 3 * k, T.t21[k], r.X1);
    s3_image(Y, C.fx2, C.fy2, C.cx2, C.cy2, u, v);
    const float e0 = __fsub_rn(u, r.p2[0]), e1 = __fsub_rn(v, r.p2[1]);
    const float err2 = cnm_f(__dadd_rn(__dadd_rn(0.0, __dmul_rn((double)e0, (double)e0)), __dmul_rn((double)e1, (double)e1)));
    return err1 < r.th1 && err2 < r.th2;
}

__device__ __forceinline__ S3Cam s3_cam(const S3Batch& B, int p)
{
    const pgorb_kf_pose& P1 = B.pose[B.pairKF1 ? B.pairKF1[p] : 0];
    const pgorb_kf_pose& P2 = B.pose[B.pairKF2 ? B.pairKF2[p] : 1];
    return S3Cam{P1.fx, P1.fy, P1.cx, P1.cy, P2.fx, P2.fy, P2.cx, P2.cy};
}

// the window of pair p: iterations [first, end), end = min(first + niter, mRansacMaxIts(N)); empty when N < minInliers
__device__ __forceinline__ void s3_window(const S3Batch& B, int p, int N, int& first, int& end, int& cap)
{
    first = max(B.dFirst ? B.dFirst[p] : B.first, 0);
    cap = B.caps[min(max(N, 0), B.cap)];
    end = (N < B.minInliers || first >= cap) ? first : min(first + B.niter, cap);
}

__global__ __launch_bounds__(S3_T) void k_sim3_hypotheses(S3Batch B)
{
    const int p = blockIdx.y, k = blockIdx.x * S3_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int N = B.nKept[p];
    int first, end, cap;
    s3_window(B, p, N, first, end, cap);
    if (k >= end - first) return;
    const int t = first + k;
    const S3Rec* R = B.recs + (int64_t)p * B.cap;
    int ia, ib, ic;
    s3_triple(B.draws + ((int64_t)p * B.maxIts + t) * 3, N, ia, ib, ic);
    ia = min(max(ia, 0), N - 1); ib = min(max(ib, 0), N - 1); ic = min(max(ic, 0), N - 1);      // (a draw >= 2^31 in the unchecked form)
    S3Sim T;
    s3_horn(s3_load(R + ia), s3_load(R + ib), s3_load(R + ic), B.fixScale, T);
    const S3Cam C = s3_cam(B, p);
    int inl = 0;
    for (int e0 = 0; e0 < N; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < N && s3_inlier(T, C, s3_load(R + e));
        inl += __popcll(__ballot(in));
    }
    if (lane == 0) {
        S3Hyp* H = B.hyps + (int64_t)p * B.niter + k;
        float4* dst = reinterpret_cast<float4*>(H);
        dst[0] = make_float4(T.R[0], T.R[1], T.R[2], T.R[3]);
        dst[1] = make_float4(T.R[4], T.R[5], T.R[6], T.R[7]);
        dst[2] = make_float4(T.R[8], T.t[0], T.t[1], T.t[2]);
        dst[3] = make_float4(T.s, __int_as_float(inl), 0.0f, 0.0f);
    }
}

__device__ __forceinline__ void s3_put_estimate(pgorb_sim3_estimate* o, const S3Sim* T)
{
#pragma unroll
    for (int k = 0; k < 9; k++) o->R12[k] = T ? T->R[k] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) o->t12[k] = T ? T->t[k] : 0.0f;
    o->s12 = T ? T->s : 0.0f;
}

__global__ __launch_bounds__(64) void k_sim3_select(S3Batch B)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int N = B.nKept[p];
    int first, end, cap;
    s3_window(B, p, N, first, end, cap);
    const S3Hyp* H = B.hyps + (int64_t)p * B.niter;
    const int bestIn = B.dBestIn ? B.dBestIn[p] : B.bestIn;
    // b[t] = max(best_in, inl[first .. t-1]); the call returns at the first t with inl[t] > minInliers && inl[t] >= b[t]; otherwise the
    // best is the LAST t with inl[t] >= b[t]
    int carry = bestIn, foundK = -1, bestK = -1;
    const int W = end - first;
    for (int k0 = 0; k0 < W && foundK < 0; k0 += 64) {
        const int k = k0 + lane;
        const int v = k < W ? H[k].inl : -1;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl = max(incl, o); }
        int excl = __shfl_up(incl, 1, 64);
        excl = lane == 0 ? carry : max(carry, excl);
        const bool ge = k < W && v >= excl;
        const unsigned long long mf = __ballot(ge && v > B.minInliers), mg = __ballot(ge);
        if (mf) {
            foundK = k0 + (int)__ffsll((long long)mf) - 1;
            bestK = foundK;
            carry = H[foundK].inl;
        } else {
            if (mg) bestK = k0 + 63 - __clzll((long long)mg);
            carry = max(carry, __shfl(incl, 63, 64));
        }
    }
    int status = 0;
    if (N < B.minInliers) status = PGORB_S3_FEW;
    const int itsAfter = foundK >= 0 ? first + foundK + 1 : end;
    if (foundK >= 0) status |= PGORB_S3_FOUND;
    else if (!(status & PGORB_S3_FEW) && itsAfter >= cap) status |= PGORB_S3_NO_MORE;

    const int64_t row = (int64_t)p * B.cap;
    int nInl = 0;
    S3Sim T;
    if (bestK >= 0) {
        const float4* s = reinterpret_cast<const float4*>(H + bestK);
        const float4 a = s[0], b = s[1], c = s[2], d = s[3];
        T.R[0] = a.x; T.R[1] = a.y; T.R[2] = a.z; T.R[3] = a.w; T.R[4] = b.x; T.R[5] = b.y; T.R[6] = b.z; T.R[7] = b.w; T.R[8] = c.x;
        T.t[0] = c.y; T.t[1] = c.z; T.t[2] = c.w; T.s = d.x;
        s3_derive(T);
    }
    if (foundK >= 0) {
        const S3Rec* R = B.recs + row;
        const S3Cam C = s3_cam(B, p);
        for (int e0 = 0; e0 < N; e0 += 64) {
            const int e = e0 + lane;
            bool in = false;
            S3Rec r;
            if (e < N) { r = s3_load(R + e); in = s3_inlier(T, C, r); }
            nInl += __popcll(__ballot(in));
            if (in) {                                                   // vbInliers[mvnIndices1[i]], LoopClosing.cc:313-318, ORBmatcher.cc:1133-1146
                B.inlier[row + r.i1] = 1;
                B.matchesOut[row + r.i1] = r.i2;
                if (B.already1) B.already1[row + r.i1] = 1;
                if (B.already2) B.already2[row + r.i2] = 1;
            }
        }
    }
    if (lane == 0) {
        if (B.best) s3_put_estimate(B.best + p, bestK >= 0 ? &T : nullptr);
        if (B.found) s3_put_estimate(B.found + p, foundK >= 0 ? &T : nullptr);
        if (B.foundSim3) {
            pgorb_sim3 o;
#pragma unroll
            for (int k = 0; k < 9; k++) { o.sR12[k] = foundK >= 0 ? T.sR12[k] : 0.0f; o.sR21[k] = foundK >= 0 ? T.sR21[k] : 0.0f; }
#pragma unroll
            for (int k = 0; k < 3; k++) { o.t12[k] = foundK >= 0 ? T.t[k] : 0.0f; o.t21[k] = foundK >= 0 ? T.t21[k] : 0.0f; }
            B.foundSim3[p] = o;
        }
        if (B.nInl) B.nInl[p] = nInl;
        if (B.info) {
            int32_t* I = B.info + (int64_t)p * PGORB_S3_INFO;
            I[0] = status; I[1] = N; I[2] = cap; I[3] = itsAfter; I[4] = nInl; I[5] = carry; I[6] = bestK >= 0 ? first + bestK : -1; I[7] = 0;
        }
    }
}

static const char* s3_params_why(const pgorb_sim3_params* P)
{
    if (!P) return "params is NULL";
    if (P->min_inliers < 3) return "min_inliers is below 3";
    if (!(P->probability > 0.0f && P->probability < 1.0f)) return "probability is outside (0, 1)";
    if (P->max_iterations < 1) return "max_iterations is below 1";
    if (P->first_iteration < 0) return "first_iteration is negative";
    if (P->niterations < 1) return "niterations is below 1";
    return nullptr;
}

extern "C" {

int pgorb_sim3_max_iterations(float probability, int min_inliers, int max_iterations, int N)
{
    return pg_sim3_cap(probability, min_inliers, max_iterations, N);
}

int pgorb_sim3_solver_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap, const int32_t* d_pair_kf1,
        const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, const int32_t* d_kf_point, const int32_t* d_matches12, int npoints,
        const pgorb_map_point* d_points, const uint8_t* d_point_bad, const pgorb_sim3_params* params, const int32_t* d_first_iteration,
        const int32_t* d_best_inliers_in, const uint32_t* d_draws, pgorb_sim3_estimate* d_found, pgorb_sim3* d_found_sim3,
        pgorb_sim3_estimate* d_best, uint8_t* d_inlier, int32_t* d_matches12_out, uint8_t* d_already1, uint8_t* d_already2, int32_t* d_info,
        int32_t* d_ninliers, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || cap < 1 || npairs < 0 || npoints < 0 ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_pose || !d_kf_point || !d_matches12 || !d_draws || !d_inlier || !d_matches12_out)) || (npoints && !d_points))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_sim3_solver_batch_device");
    if (const char* why = s3_params_why(params)) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_sim3_solver: ") + why).c_str());
    if (cap > S3_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_sim3_solver: more than 16000 keypoints per frame");
    if (params->max_iterations > PGORB_SIM3_MAX_ITERATIONS) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_sim3_solver: max_iterations above PGORB_SIM3_MAX_ITERATIONS");
    if (!npairs) return 0;
    S3Batch B;
    B.nlevels = pgorb_levels(c);
    memset(B.sigma2, 0, sizeof(B.sigma2));
    if (!(B.nlevels > 0) || B.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, B.sigma2, nullptr) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    hipStream_t s = (hipStream_t)stream;
    int rc = pg_ctx_sim3_caps(c, params->probability, params->min_inliers, params->max_iterations, S3_MAX_N, &B.caps);
    if (rc) return rc;
    B.niter = std::min(params->niterations, params->max_iterations);       // no window is longer than the cap
    PgCarve L;
    const size_t oRec = L.take((size_t)npairs * cap * sizeof(S3Rec)), oHyp = L.take((size_t)npairs * B.niter * sizeof(S3Hyp)),
                 oN = L.take((size_t)npairs * 4);
    void* scr;
    if ((rc = pg_ctx_scratch(c, L.o, s, &scr))) return rc;
    B.K = d_kps; B.n = d_n; B.cap = cap; B.pairKF1 = d_pair_kf1; B.pairKF2 = d_pair_kf2; B.pose = d_pose; B.kfPoint = d_kf_point;
    B.matches12 = d_matches12; B.npoints = npoints; B.pts = d_points; B.pbad = d_point_bad;
    B.minInliers = params->min_inliers; B.fixScale = params->fix_scale ? 1 : 0; B.first = params->first_iteration;
    B.bestIn = params->best_inliers_in; B.maxIts = params->max_iterations;
    B.dFirst = d_first_iteration; B.dBestIn = d_best_inliers_in; B.draws = d_draws;
    B.recs = (S3Rec*)((uint8_t*)scr + oRec); B.hyps = (S3Hyp*)((uint8_t*)scr + oHyp); B.nKept = (int32_t*)((uint8_t*)scr + oN);
    B.found = d_found; B.foundSim3 = d_found_sim3; B.best = d_best; B.inlier = d_inlier; B.matchesOut = d_matches12_out;
    B.already1 = d_already1; B.already2 = d_already2; B.info = d_info; B.nInl = d_ninliers;
    hipLaunchKernelGGL(k_sim3_prepare, dim3((unsigned)npairs), dim3(S3_T), 0, s, B);
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((B.niter + S3_WAVES - 1) / S3_WAVES), (unsigned)npairs), dim3(S3_T), 0, s, B);
    hipLaunchKernelGGL(k_sim3_select, dim3((unsigned)npairs), dim3(64), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "a Sim3Solver kernel launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool s3_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

int pgorb_sim3_solver(pgorb_ctx* c, const pgorb_keypoint* kps1, int n1, const pgorb_kf_pose* pose1, const int32_t* kf_point1,
        const pgorb_keypoint* kps2, int n2, const pgorb_kf_pose* pose2, const int32_t* kf_point2, const int32_t* matches12, int npoints,
        const pgorb_map_point* points, const uint8_t* point_bad, const pgorb_sim3_params* params, const uint32_t* draws,
        pgorb_sim3_estimate* found, pgorb_sim3* found_sim3, pgorb_sim3_estimate* best, uint8_t* inlier, int32_t* matches12_out,
        uint8_t* already1, uint8_t* already2, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    if (n1 < 0 || n2 < 0 || npoints < 0) why = "a count is negative";
    else if (!pose1 || !pose2 || !params || !draws || (n1 && (!kps1 || !kf_point1 || !matches12 || !inlier || !matches12_out)) ||
             (n2 && (!kps2 || !kf_point2)) || (npoints && !points)) why = "an array that is read is NULL";
    else why = s3_params_why(params);
    if (!why && (!s3_all_finite(pose1->Tcw, 12) || !s3_all_finite(&pose1->fx, 4) || !s3_all_finite(pose2->Tcw, 12) || !s3_all_finite(&pose2->fx, 4)))
        why = "a pose or a camera is not finite";
    for (int i = 0; !why && i < n1; i++)
        if (kf_point1[i] < -1 || kf_point1[i] >= npoints) why = "a slot's point index is out of range";
    for (int i = 0; !why && i < n2; i++)
        if (kf_point2[i] < -1 || kf_point2[i] >= npoints) why = "a slot's point index is out of range";
    for (int i = 0; !why && i < n1; i++) {
        const int j = matches12[i];
        if (j < -1 || j >= n2) { why = "matches12 is outside [-1, n2)"; break; }
        if (j < 0 || kf_point1[i] < 0 || kf_point2[j] < 0) continue;
        if (kps1[i].octave < 0 || kps1[i].octave >= nlevels || kps2[j].octave < 0 || kps2[j].octave >= nlevels) why = "an octave is outside the context's levels";
        else if (!s3_all_finite(points[kf_point1[i]].pos, 3) || !s3_all_finite(points[kf_point2[j]].pos, 3)) why = "a referenced point is not finite";
    }
    if (!why && params->max_iterations <= PGORB_SIM3_MAX_ITERATIONS)
        for (int64_t k = 0; k < (int64_t)params->max_iterations * 3; k++)
            if (draws[k] >= 0x80000000u) { why = "a draw is not below 2^31"; break; }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_sim3_solver: ") + why).c_str());
    if (n1 > S3_MAX_N || n2 > S3_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_sim3_solver: more than 16000 keypoints per frame");
    if (params->max_iterations > PGORB_SIM3_MAX_ITERATIONS) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_sim3_solver: max_iterations above PGORB_SIM3_MAX_ITERATIONS");
    const int cap = std::max(std::max(n1, n2), 1), np = std::max(npoints, 1);
    const size_t nd = (size_t)params->max_iterations * 3 * 4;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)2 * cap * sizeof(pgorb_keypoint)), oPose = s.region(PG_UP, 2 * sizeof(pgorb_kf_pose)),
                 oS = s.region(PG_UP, (size_t)2 * cap * 4), oM = s.region(PG_UP, (size_t)cap * 4), oP = s.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)),
                 oB = s.region(PG_UP, point_bad ? np : 0), oD = s.region(PG_UP, nd),
                 oF = s.region(PG_DOWN, sizeof(pgorb_sim3_estimate)), oFS = s.region(PG_DOWN, sizeof(pgorb_sim3)), oBest = s.region(PG_DOWN, sizeof(pgorb_sim3_estimate)),
                 oI = s.region(PG_DOWN, cap), oMO = s.region(PG_DOWN, (size_t)cap * 4), oA1 = s.region(PG_DOWN, cap), oA2 = s.region(PG_DOWN, cap),
                 oR = s.region(PG_DOWN, 64);
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
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    if (point_bad) s.put(oB, point_bad, npoints, 0, np);
    s.put(oD, draws, nd);
    int32_t* R = s.dev<int32_t>(oR);                                    // ninliers, -, info[8] from R + 2
    if ((rc = s.run([&] {
            const int32_t* N = s.dev<int32_t>(oN);
            return pgorb_sim3_solver_batch_device(c, s.dev<pgorb_keypoint>(oK), N, cap, N + 2, N + 3, 1, s.dev<pgorb_kf_pose>(oPose),
                                                  s.dev<int32_t>(oS), s.dev<int32_t>(oM), npoints, s.dev<pgorb_map_point>(oP),
                                                  point_bad ? s.dev(oB) : nullptr, params, nullptr, nullptr, s.dev<uint32_t>(oD),
                                                  s.dev<pgorb_sim3_estimate>(oF), s.dev<pgorb_sim3>(oFS), s.dev<pgorb_sim3_estimate>(oBest),
                                                  s.dev(oI), s.dev<int32_t>(oMO), s.dev(oA1), s.dev(oA2), R + 2, R, nullptr); }))) return rc;
    if (found) memcpy(found, s.host(oF), sizeof(pgorb_sim3_estimate));
    if (found_sim3) memcpy(found_sim3, s.host(oFS), sizeof(pgorb_sim3));
    if (best) memcpy(best, s.host(oBest), sizeof(pgorb_sim3_estimate));
    if (n1) { memcpy(inlier, s.host(oI), n1); memcpy(matches12_out, s.host(oMO), (size_t)n1 * 4); }
    if (already1 && n1) memcpy(already1, s.host(oA1), n1);
    if (already2 && n2) memcpy(already2, s.host(oA2), n2);
    const int32_t* r = s.host<int32_t>(oR);
    if (info) memcpy(info, r + 2, PGORB_S3_INFO * 4);
    return r[0];
}

}  // extern "C"
