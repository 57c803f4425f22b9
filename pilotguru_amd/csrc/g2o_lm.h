// g2o_lm.h -- the g2o and Eigen machinery that the five optimisers share (pose_opt.hip, optimize_sim3.hip, local_ba.hip,
// essential_graph.hip, global_ba.hip; g2o_se3.h and g2o_sim3.h build on it), each reading in ONE copy: the deterministic block
// reductions, RobustKernelHuber, the finite test, LinearSolverDense's LDLT, OptimizationAlgorithmLevenberg's step control, Eigen's
// 3 x 3 inverse and Eigen's quaternion.  In double and in the sources' operation order: DESIGN.md section 4 lists the readings.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define G2O_DBL_MAX 1.7976931348623157e308        /* std::numeric_limits<double>::max() */
__device__ __forceinline__ bool g2o_finite(double v) { return fabs(v) <= G2O_DBL_MAX; }      // g2o_isfinite; false for a NaN

// ---- reductions over a workgroup of 256 threads (four waves), through the caller's LDS.  The fixed tree: a xor butterfly inside the
// wave (a + b is b + a bit for bit, so every lane ends with the same value), then (w0 + w1) + (w2 + w3).  One barrier after the
// write and one after the read: a call may follow another on the same `part` at once, and what a thread wrote to LDS or to memory
// before the call is published to the workgroup when the call returns.
template <class T>
__device__ __forceinline__ T g2o_block_sum(T* part /* LDS [4] */, T v)                              // T = int or double
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const T r = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ double g2o_block_max(double* part /* LDS [4] */, double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
    __syncthreads();
    return r;
}
// N sums at once: red[k] = the tree over every thread's v[k]
template <int N>
__device__ __forceinline__ void g2o_block_sum_n(double (&part)[4][N], double (&red)[N], double (&v)[N])
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += __shfl_xor(v[k], m, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; k++) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < N) red[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    __syncthreads();
}

// ---- the edge's scalar pieces
// chi2 = _error.dot(information * _error), information = w * I
__device__ __forceinline__ double g2o_chi2(double e0, double e1, double w) { return e0 * (w * e0) + e1 * (w * e1); }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
__device__ __forceinline__ void g2o_huber(double e, double delta, double& rho0, double& rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { rho0 = e; rho1 = 1.0; }
    else {
        const double sqrte = __dsqrt_rn(e);
        rho0 = 2.0 * sqrte * delta - dsqr;
        rho1 = delta / sqrte;
    }
}

// ---- LinearSolverDense::solve (linear_solver_dense.h:104-112): an LDLT of the N x N in index order (no pivoting: DESIGN.md
// section 4); false = a factor is not positive
template <int N>
__device__ __forceinline__ bool g2o_ldlt_solve(const double (&H)[N][N], const double (&b)[N], double (&x)[N])
{
    double L[N][N], d[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = H[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= (L[j][k] * L[j][k]) * d[k];
        d[j] = s;
        ok = ok && (s > 0.0);
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double t = H[j][i];
#pragma unroll
            for (int k = 0; k < j; k++) t -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) t -= L[i][k] * y[k];
        y[i] = t;
    }
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = y[i] / d[i];
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double t = y[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) t -= L[k][i] * x[k];
        x[i] = t;
    }
    return ok;
}

// The dense N x N system out of a reduction's sums: the upper triangle by rows, mirrored (g2o keeps the upper block and the solver
// copies it across), then b
template <int N>
__device__ __forceinline__ void g2o_dense_system(const double* red, double (&H)[N][N], double (&b)[N])
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++) { H[i][j] = red[k]; H[j][i] = red[k]; k++; }
#pragma unroll
    for (int i = 0; i < N; i++) b[i] = red[N * (N + 1) / 2 + i];
}
// computeLambdaInit's largest diagonal entry
template <int N>
__device__ __forceinline__ double g2o_max_diagonal(const double (&H)[N][N])
{
    double md = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) md = fmax(fabs(H[j][j]), md);
    return md;
}

// One trial of the dense N x N solvers: setLambda, solve, and the x'(lambda x + b) of computeScale.  A failed factorisation leaves
// x = 0, so the trial stays at the estimate.  fixLast: VertexSim3Expmap::oplusImpl under _fix_scale writes 0 into the solver's x,
// and computeScale sees it.
template <int N>
__device__ __forceinline__ bool g2o_dense_trial(const double (&H)[N][N], const double (&b)[N], double lambda, bool fixLast, double (&x)[N], double& scale)
{
    double Hl[N][N];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) Hl[i][j] = i == j ? H[i][j] + lambda : H[i][j];
    const bool ok2 = g2o_ldlt_solve(Hl, b, x);
    if (!ok2) {
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = 0.0;
    }
    if (fixLast) x[N - 1] = 0.0;
    scale = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) scale += x[j] * (lambda * x[j] + b[j]);
    return ok2;
}

// ---- OptimizationAlgorithmLevenberg::solve's step control (optimization_algorithm_levenberg.cpp:61-189)
#define G2O_LM_TRIALS 10                          /* _maxTrialsAfterFailure */
struct G2oLm { double lambda; int32_t ni, nBad; };

// the start of the first iteration: lambda = computeLambdaInit, _ni = 2; SparseOptimizer::optimize's count of bad iterations restarts
__device__ __forceinline__ void g2o_lm_begin(G2oLm& L, double lambdaInit) { L.lambda = lambdaInit; L.ni = 2; L.nBad = 0; }
// computeLambdaInit without a user value: _tau * the largest diagonal entry of the active vertices' blocks
__device__ __forceinline__ double g2o_lm_lambda_init(double maxDiagonal) { return 1e-5 * maxDiagonal; }

// The decision after a trial (:110-150).  tempChi = the trial's activeRobustChi2, DBL_MAX when the solve failed; scale = the sum
// x'(lambda x + b), to which computeScale adds 1e-3.  true = accepted: currentChi is the trial's and the caller's discardTop makes
// the trial the estimate; false: the caller's pop keeps the estimate.
__device__ __forceinline__ bool g2o_lm_decide(G2oLm& L, double& currentChi, double tempChi, bool ok2, double scale, double& rho)
{
    if (!ok2) tempChi = G2O_DBL_MAX;
    rho = (currentChi - tempChi) / (scale + 1e-3);
    if (rho > 0.0 && g2o_finite(tempChi)) {
        const double t = 2.0 * rho - 1.0;
        double alpha = 1.0 - (t * t) * t;                               // pow(2 * rho - 1, 3) read as two products
        alpha = fmin(alpha, 2.0 / 3.0);
        L.lambda *= fmax(1.0 / 3.0, alpha); L.ni = 2; currentChi = tempChi;
        return true;
    }
    L.lambda *= (double)L.ni; L.ni *= 2;
    return false;
}
// the trial loop's condition: while (rho < 0 && qmax < _maxTrialsAfterFailure)
__device__ __forceinline__ bool g2o_lm_again(double rho, int qmax) { return rho < 0.0 && qmax < G2O_LM_TRIALS; }

// The end of an iteration, true = stop: Terminate (qmax == _maxTrialsAfterFailure || rho == 0), then SparseOptimizer::optimize's
// rule that three iterations in a row which gain less than 1e-3 of their chi2 end it (the project's reading: DESIGN.md section 4)
__device__ __forceinline__ bool g2o_lm_stop(G2oLm& L, double iniChi, double currentChi, int qmax, double rho)
{
    if (qmax == G2O_LM_TRIALS || rho == 0.0) return true;
    if ((iniChi - currentChi) * 1e3 < iniChi) L.nBad++; else L.nBad = 0;
    return L.nBad >= 3;
}

// ---- Eigen
// the fixed-size 3 x 3 inverse (Inverse.h compute_inverse<Matrix3d>): cofactors, the determinant from the first cofactor column, no test
__device__ __forceinline__ void g2o_inverse3(const double (&D)[9], double (&I)[9])
{
#define G2O_COF(i, j) (D[((i + 1) % 3) * 3 + (j + 1) % 3] * D[((i + 2) % 3) * 3 + (j + 2) % 3] - D[((i + 1) % 3) * 3 + (j + 2) % 3] * D[((i + 2) % 3) * 3 + (j + 1) % 3])
    const double c00 = G2O_COF(0, 0), c10 = G2O_COF(1, 0), c20 = G2O_COF(2, 0);
    const double det = (c00 * D[0] + c10 * D[3]) + c20 * D[6];
    const double inv = 1.0 / det;
    I[0] = c00 * inv; I[1] = c10 * inv; I[2] = c20 * inv;
    I[3] = G2O_COF(0, 1) * inv; I[4] = G2O_COF(1, 1) * inv; I[5] = G2O_COF(2, 1) * inv;
    I[6] = G2O_COF(0, 2) * inv; I[7] = G2O_COF(1, 2) * inv; I[8] = G2O_COF(2, 2) * inv;
#undef G2O_COF
}

// The quaternion, over any struct with the coefficients qx, qy, qz, qw (PoSE3, OsSim).
// Quaterniond(Matrix3d); m row-major
template <class Q>
__device__ __forceinline__ void g2o_quat_from_matrix(const double (&m)[9], Q& P)
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
// the same of the rotation in rows 0-2 of a row-major float [R | t] with four columns (Converter::toMatrix3d of a cv::Mat pose)
template <class Q>
__device__ __forceinline__ void g2o_quat_from_pose(const float* T, Q& P)
{
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
    g2o_quat_from_matrix(R, P);
}

// Quaternion::toRotationMatrix, row-major
template <class Q>
__device__ __forceinline__ void g2o_matrix_from_quat(const Q& P, double (&m)[9])
{
    const double tx = 2.0 * P.qx, ty = 2.0 * P.qy, tz = 2.0 * P.qz;
    const double twx = tx * P.qw, twy = ty * P.qw, twz = tz * P.qw, txx = tx * P.qx, txy = ty * P.qx, txz = tz * P.qx;
    const double tyy = ty * P.qy, tyz = tz * P.qy, tzz = tz * P.qz;
    m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy;
    m[3] = txy + twz; m[4] = 1.0 - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy; m[7] = tyz + twx; m[8] = 1.0 - (txx + tyy);
}

// quaternion * vector: uv = vec x v; uv += uv; v + w * uv + vec x uv
template <class Q>
__device__ __forceinline__ void g2o_rotate(const Q& P, double X, double Y, double Z, double& rx, double& ry, double& rz)
{
    double ux = P.qy * Z - P.qz * Y, uy = P.qz * X - P.qx * Z, uz = P.qx * Y - P.qy * X;
    ux += ux; uy += uy; uz += uz;
    rx = (X + P.qw * ux) + (P.qy * uz - P.qz * uy);
    ry = (Y + P.qw * uy) + (P.qz * ux - P.qx * uz);
    rz = (Z + P.qw * uz) + (P.qx * uy - P.qy * ux);
}
