// global_ba.hip -- Optimizer::GlobalBundleAdjustemnt on gfx950: the bundle adjustment of every key frame and every map point, ONE
// problem spread over many workgroups and a fixed sequence of launches on the caller's stream.
//
// Restates (thirdparty/orb-slam2, thirdparty/g2o):
//   Optimizer::GlobalBundleAdjustemnt / BundleAdjustment   src/Optimizer.cc:41-46, :49-237 (monocular edges only, mvuRight < 0)
//   Converter::toSE3Quat / toCvMat                src/Converter.cc
//   VertexSE3Expmap / VertexSBAPointXYZ (oplus)   g2o/types/types_six_dof_expmap.h, types_sba.h
//   EdgeSE3ProjectXYZ                             g2o/types/types_six_dof_expmap.{h,cpp} (computeError, linearizeOplus :103-139)
//   BaseBinaryEdge::constructQuadraticForm        g2o/core/base_binary_edge.hpp:60-116
//   RobustKernelHuber::robustify                  g2o/core/robust_kernel_impl.cpp:78-91 (delta = (float)sqrt(5.99), :57)
//   BlockSolver_6_3 (buildSystem, setLambda, solve)   g2o/core/block_solver.hpp:353-589
//   OptimizationAlgorithmLevenberg::solve         g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   KeyFrame::SetPose                             src/KeyFrame.cc
// in double, under the readings of DESIGN.md sections 4 and 5 (the local-bundle-adjustment rows and the global ones).  The edge
// arithmetic is local_ba.hip's: both call g2o_se3.h's one copy of EdgeSE3ProjectXYZ's error and linearisation, of toSE3Quat and of
// SetPose (pose_opt.hip shares all but the linearisation).  Huber, the block reductions, the 3 x 3 inverse and Levenberg's step
// control (here on the state record: k_gba_begin, k_gba_decide) are g2o_lm.h's, shared with pose_opt.hip, optimize_sim3.hip,
// local_ba.hip and essential_graph.hip.  LinearSolverEigen is READ, as in essential_graph.hip, as a Cholesky L L' in
// index order on a block skyline (row i keeps its 6 x 6 blocks from the lowest-indexed camera that shares a point with it to i).
//
// Launches (no host round trip, no cooperative launch, no wait between workgroups; every loop is bounded by a capacity or a constant):
//   k_gba_prepare    one workgroup: the flags, the edge records, each camera's edge list in CSR order (= points in table order, a
//                    point's edges in CSR order: the order every per-camera sum runs in), the system indices, the envelope.
//   per iteration:
//   k_gba_linearize  all CUs.  Workgroups [0, ptBlocks): a POINT belongs to one thread, which linearises its edges in CSR order and
//                    sums Hll, bl and its chi2 in that order, and leaves each edge's W = Jj' wOmega Ji.  Workgroups behind them: a
//                    camera BLOCK ROW belongs to one workgroup, which recomputes its own edges' Jacobians (nothing another
//                    workgroup writes in this launch is read), stages 256 edges at a time in LDS, and lane (a, b) sums entry (a, b)
//                    of Hpp, lane 36 + a entry a of bp, in list order.  chi2 and the diagonal maximum leave as per-workgroup partials.
//   k_gba_begin      one workgroup: the partials in one fixed tree; the chi2 the iteration starts from, lambda at iteration 0.
//   per trial (at most 10, g2o's _maxTrialsAfterFailure):
//   k_gba_schur      one workgroup per block row i: Dinv = (Hll + lambda I)^-1 of the row's points, 64 at a time in LDS, then the
//                    walk of camera i's edge list: block (i, j <= i) -= W_jp Dinv_p W_ip' entry by entry, and bschur.  Entry (a, b)
//                    of block (i, j) belongs to thread (j mod 7) * 36 + a * 6 + b, so every entry sees its updates in list order.
//   k_gba_solve      one workgroup: the block skyline's Cholesky in index order (the diagonal block by 36 lanes of one wave, the
//                    panel of the pivot column staged in LDS), forward and back solve, oplus into the trial cameras, and the camera
//                    half of computeScale.
//   k_gba_try        all CUs, a point a thread: Dinv again, xl = Dinv (bl - sum W' xp), the trial point, its edges' chi2 at the trial
//                    estimates and its computeScale terms; per-workgroup partials.
//   k_gba_decide     one workgroup: the partials in one fixed tree, rho, accept (the estimate buffers swap roles) or reject, lambda
//                    and nu, and at the end of the trial loop the stop rules.  All of it stays in the state record in the arena.
//   k_gba_finish     all CUs: pose_out, pos_out, the done flags, chi2, the table in place, info.
// The decision is a launch of its own and not the head of the next all-CU kernel: a state record that many workgroups read must not be
// written in the same launch.  That is 42 launches an iteration, not the 31 of the sketch: at 20 iterations 842, ~3.6 ms when idle.
// A kernel behind the problem's stop flag, or behind the end of its iteration, returns at once.
#include "kf_window.h"
#include "g2o_se3.h"
#include <math.h>
#include <string>
#include <vector>

#define GBA_T 256
#define GBA_PREP_T 1024
#define GBA_CHUNKS 256            // k_gba_prepare splits the observations into this many runs to build the cameras' lists in order
#define GBA_MAX_N 16000           // keypoints per frame, as for the matchers
#define GBA_PANEL 64              // blocks of a pivot column kept in LDS
#define GBA_DELTA ((double)0x1.3945f6p+1f)        /* const float thHuber2D = sqrt(5.99) = 2.4474475f (Optimizer.cc:57) */

struct GbaEdge { int32_t frame /* < 0: the observation is no edge */, pt, row, pad; float ox, oy, w, pad1; };
static_assert(sizeof(GbaEdge) == 32, "two dwordx4");
struct GbaCam { PoSE3 est[2]; double fx, fy, cx, cy; };
struct GbaState {
    int32_t status, stop, nE, nPts, nVert, nFree, env, its, trials, iter, qmax, ok2, cur, pad;
    G2oLm lm;
    double currentChi, iniChi, camScale;
};
// a point's doubles: Hll, bl
enum { GP_HLL = 0, GP_BL = 9, GBA_PT_D = 12 };

struct GbaArgs {
    const pgorb_keypoint* K; const int32_t* n; int cap, nkf;
    const pgorb_kf_pose* pose; const uint8_t* kfBad; const uint8_t* id0;
    int npoints; pgorb_map_point* pts; const uint8_t* ptBad; const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs;
    int iterations, robust, inPlace, nlevels;
    float invSigma2[PG_MAXL + 1];
    pgorb_kf_pose* poseOut; float* posOut; uint8_t* kfDone; uint8_t* ptDone; float* chi2; int32_t* info;
    // the arena
    int envCap, ptBlocks;
    GbaState* st; GbaEdge* eI; double* eW; double* pX; double* pH; int32_t* pInc;
    GbaCam* cams; int32_t* sys; int32_t* rowKf; int32_t* camStart; int32_t* camEdge; int32_t* chunkCnt; int32_t* tmp;
    int32_t* first; int32_t* off; int32_t* colStart; int32_t* colRows;
    double* Hpp; double* bp; double* bs; double* x; double* A;
    double* chiPart; double* maxPart; double* scPart;
};

__device__ __forceinline__ bool gba_bad(const GbaArgs& G, int f) { return G.kfBad && G.kfBad[f]; }
__device__ __forceinline__ double* gba_x(const GbaArgs& G, int buf, int p) { return G.pX + ((int64_t)buf * max(G.npoints, 1) + p) * 3; }
__device__ __forceinline__ int2 gba_range(const GbaArgs& G, int p)
{
    int a = G.obsStart[p], b = G.obsStart[p + 1];
    if (a < 0 || b > G.nobs || b < a) a = b = 0;                        // a list outside the arrays is an empty list
    return make_int2(a, b);
}

// n partials: thread t takes t, t + 256, ... in that order, then the tree
__device__ __forceinline__ double gba_reduce_sum(double* part, const double* v, int n)
{
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += GBA_T) acc += v[k];
    return g2o_block_sum(part, acc);
}

// exclusive scan of in[0 .. n) into out (may be in), every thread of the workgroup calls it; returns the total
__device__ int gba_scan(const int32_t* in, int32_t* out, int n, int32_t* part /* LDS [T + 1] */)
{
    const int T = blockDim.x, t = threadIdx.x;
    const int chunk = (n + T - 1) / T, k0 = min(t * chunk, n), k1 = min(k0 + chunk, n);
    int s = 0;
    for (int k = k0; k < k1; k++) s += in[k];
    __syncthreads();
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < T; k++) { const int v = part[k]; part[k] = run; run += v; }
        part[T] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int k = k0; k < k1; k++) { const int v = in[k]; out[k] = run; run += v; }
    const int total = part[T];
    __syncthreads();
    return total;
}

// ---- the sets of Optimizer.cc:71-110 as flags, and the lists the solver walks
__global__ __launch_bounds__(GBA_PREP_T) void k_gba_prepare(GbaArgs G)
{
    __shared__ int32_t part[GBA_PREP_T + 1];
    const int tid = threadIdx.x, T = GBA_PREP_T, nkf = G.nkf, npoints = G.npoints, nobs = G.nobs;
    // the vertices (:71-83): every key frame that is not bad
    for (int f = tid; f < nkf; f += T) {
        const pgorb_kf_pose in = G.pose[f];
        GbaCam C;
        memset(&C, 0, sizeof(C));
        C.est[0].qw = 1.0;
        if (!gba_bad(G, f)) C.est[0] = po_from_pose(in);
        C.est[1] = C.est[0];
        C.fx = (double)in.fx; C.fy = (double)in.fy; C.cx = (double)in.cx; C.cy = (double)in.cy;
        G.cams[f] = C;
        G.tmp[f] = gba_bad(G, f) ? 0 : 1;
    }
    for (int k = tid; k < nobs; k += T) G.eI[k].frame = -1;
    __syncthreads();
    const int nVert = gba_scan(G.tmp, G.tmp, nkf, part);
    // the edges (:105-110): every observation of a point that is not bad in a key frame that is not bad; the included points (:175-183)
    int cntE = 0, cntP = 0;
    for (int p = tid; p < npoints; p += T) {
        const int2 r = gba_range(G, p);
        const bool live = !(G.ptBad && G.ptBad[p]);
        int cnt = 0;
        for (int k = r.x; k < r.y; k++) {
            const int f = G.obsFrame[k], i = G.obsIdx[k];
            bool ok = live && f >= 0 && f < nkf && !gba_bad(G, f);
            if (ok) ok = i >= 0 && i < min(max(G.n[f], 0), G.cap);
            GbaEdge e;
            e.frame = -1; e.pt = p; e.row = -1; e.pad = 0; e.ox = e.oy = e.w = e.pad1 = 0.0f;
            if (ok) {
                const pgorb_keypoint kp = G.K[(int64_t)f * G.cap + i];
                if (kp.octave >= 0 && kp.octave < G.nlevels) { e.frame = f; e.ox = kp.x; e.oy = kp.y; e.w = G.invSigma2[kp.octave]; cnt++; }
            }
            G.eI[k] = e;
        }
        G.pInc[p] = cnt > 0;
        cntE += cnt; cntP += cnt > 0 ? 1 : 0;
        const pgorb_map_point P = G.pts[p];
#pragma unroll
        for (int m = 0; m < 3; m++) { gba_x(G, 0, p)[m] = (double)P.pos[m]; gba_x(G, 1, p)[m] = (double)P.pos[m]; }
    }
    __syncthreads();
    part[tid] = cntE;
    __syncthreads();
    int nE = 0, nPts = 0;
    if (tid == 0) { for (int k = 0; k < T; k++) nE += part[k]; part[T] = nE; }
    __syncthreads();
    nE = part[T];
    __syncthreads();
    part[tid] = cntP;
    __syncthreads();
    if (tid == 0) { for (int k = 0; k < T; k++) nPts += part[k]; part[T] = nPts; }
    __syncthreads();
    nPts = part[T];
    __syncthreads();
    // each camera's edges in CSR order: run c of the observations counts its edges per camera, a scan over the runs gives every run its
    // place in every list, and the run writes its edges there
    const int run = (nobs + GBA_CHUNKS - 1) / GBA_CHUNKS;
    for (int64_t q = tid; q < (int64_t)GBA_CHUNKS * nkf; q += T) G.chunkCnt[q] = 0;
    __syncthreads();
    if (tid < GBA_CHUNKS)
        for (int k = tid * run, k1 = min(k + run, nobs); k < k1; k++) {
            const int f = G.eI[k].frame;
            if (f >= 0) G.chunkCnt[(int64_t)tid * nkf + f]++;
        }
    __syncthreads();
    for (int f = tid; f < nkf; f += T) {
        int at = 0;
        for (int c = 0; c < GBA_CHUNKS; c++) { const int v = G.chunkCnt[(int64_t)c * nkf + f]; G.chunkCnt[(int64_t)c * nkf + f] = at; at += v; }
        G.camStart[f] = at;
        // free and active: not bad, not the key frame with mnId 0 (:79), with an edge (initializeOptimization drops the others)
        G.tmp[f] = (!gba_bad(G, f) && !(G.id0 && G.id0[f]) && at > 0) ? 1 : 0;
    }
    __syncthreads();
    const int nFree = gba_scan(G.tmp, G.sys, nkf, part);
    for (int f = tid; f < nkf; f += T) {
        if (G.tmp[f]) G.rowKf[G.sys[f]] = f; else G.sys[f] = -1;
    }
    __syncthreads();
    const int total = gba_scan(G.camStart, G.camStart, nkf, part);
    if (tid == 0) G.camStart[nkf] = total;
    __syncthreads();
    if (tid < GBA_CHUNKS)
        for (int k = tid * run, k1 = min(k + run, nobs); k < k1; k++) {
            const int f = G.eI[k].frame;
            if (f >= 0) G.camEdge[G.camStart[f] + G.chunkCnt[(int64_t)tid * nkf + f]++] = k;
        }
    for (int k = tid; k < nobs; k += T) {
        const int f = G.eI[k].frame;
        if (f >= 0) G.eI[k].row = G.sys[f];
    }
    __syncthreads();
    // the envelope: row r reaches back to the lowest-indexed camera that shares a point with it
    for (int r = tid; r < nFree; r += T) {
        const int f = G.rowKf[r];
        int lo = r;
        for (int e = G.camStart[f]; e < G.camStart[f + 1]; e++) {
            const int2 rg = gba_range(G, G.eI[G.camEdge[e]].pt);
            for (int k = rg.x; k < rg.y; k++) {
                const GbaEdge E = G.eI[k];
                if (E.frame >= 0 && E.row >= 0) lo = min(lo, E.row);
            }
        }
        G.first[r] = lo;
        G.tmp[r] = r - lo + 1;
    }
    __syncthreads();
    const int env = gba_scan(G.tmp, G.off, nFree, part);
    if (tid == 0) G.off[nFree] = env;
    const bool fits = env <= G.envCap;
    // the rows below the diagonal that reach column k, in increasing row: a column's thread counts them, then writes them
    for (int k = tid; k < nFree; k += T) {
        int m = 0;
        if (fits)
            for (int r = k + 1; r < nFree; r++) m += G.first[r] <= k ? 1 : 0;
        G.tmp[k] = m;
    }
    __syncthreads();
    gba_scan(G.tmp, G.colStart, nFree, part);
    if (tid == 0) G.colStart[nFree] = fits ? env - nFree : 0;
    if (fits)
        for (int k = tid; k < nFree; k += T) {
            int at = G.colStart[k];
            for (int r = k + 1; r < nFree; r++)
                if (G.first[r] <= k) G.colRows[at++] = r;
        }
    if (tid == 0) {
        GbaState S;
        memset(&S, 0, sizeof(S));
        S.nE = nE; S.nPts = nPts; S.nVert = nVert; S.nFree = nFree; S.env = env;
        if (nE == 0 || nFree == 0) S.status = PGORB_GBA_NOTHING;
        else if (!fits) S.status = PGORB_GBA_LIMIT;
        S.stop = (S.status || G.iterations <= 0) ? 1 : 0;
        S.lm.ni = 2;
        *G.st = S;
    }
}

// one edge at P and X through g2o_se3.h's single copies: the linearisation, and the error alone
__device__ __forceinline__ void gba_linearize_edge(const PoSE3& P, const GbaCam& C, const double* X, const GbaEdge& e, bool robust, PoLin& L)
{
    po_linearize_xyz(P, C.fx, C.fy, C.cx, C.cy, X, (double)e.ox, (double)e.oy, (double)e.w, robust, GBA_DELTA, L);
}
__device__ __forceinline__ void gba_error(const PoSE3& P, const GbaCam& C, const double* X, const GbaEdge& e, double& e0, double& e1)
{
    double x, y, z;
    po_error(P, C.fx, C.fy, C.cx, C.cy, X[0], X[1], X[2], (double)e.ox, (double)e.oy, x, y, z, e0, e1);
}
// Dinv = (Hll + lambda I)^-1 of point p (setLambda on the landmark diagonal, block_solver.hpp:385-395)
__device__ __forceinline__ void gba_dinv(const GbaArgs& G, int p, double lambda, double (&I)[9])
{
    const double* PH = G.pH + (int64_t)p * GBA_PT_D;
    double D[9];
#pragma unroll
    for (int m = 0; m < 9; m++) D[m] = PH[GP_HLL + m];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    g2o_inverse3(D, I);
}

struct GbaLinShared { double part[GBA_T / 64]; double J[GBA_T][15]; double dg[6]; };

__global__ __launch_bounds__(GBA_T) void k_gba_linearize(GbaArgs G)
{
    __shared__ GbaLinShared S;
    const GbaState st = *G.st;
    if (st.stop) return;
    const int tid = threadIdx.x, cur = st.cur;
    const bool robust = G.robust != 0;
    if ((int)blockIdx.x < G.ptBlocks) {
        // computeActiveErrors, activeRobustChi2, buildSystem: the landmark half, a point a thread
        const int p = blockIdx.x * GBA_T + tid;
        double chiP = 0.0, maxd = 0.0;
        if (p < G.npoints && G.pInc[p]) {
            const double* X = gba_x(G, cur, p);
            const int2 r = gba_range(G, p);
            double Hl[9], bl[3];
#pragma unroll
            for (int m = 0; m < 9; m++) Hl[m] = 0.0;
            bl[0] = bl[1] = bl[2] = 0.0;
            for (int k = r.x; k < r.y; k++) {
                const GbaEdge e = G.eI[k];
                if (e.frame < 0) continue;
                const GbaCam& C = G.cams[e.frame];
                const PoSE3 P = C.est[cur];
                PoLin L;
                gba_linearize_edge(P, C, X, e, robust, L);
                chiP += L.rho0;
                double Ji0[3], Ji1[3];
                po_point_jacobian(P, C.fx, C.fy, L, Ji0, Ji1);
#pragma unroll
                for (int a = 0; a < 3; a++) {
#pragma unroll
                    for (int b = 0; b < 3; b++) Hl[a * 3 + b] += (Ji0[a] * L.wO) * Ji0[b] + (Ji1[a] * L.wO) * Ji1[b];
                    bl[a] += Ji0[a] * L.r0 + Ji1[a] * L.r1;
                }
                double* W = G.eW + (int64_t)k * 18;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int m = 0; m < 3; m++) W[a * 3 + m] = (L.Jj0[a] * L.wO) * Ji0[m] + (L.Jj1[a] * L.wO) * Ji1[m];
            }
            double* PH = G.pH + (int64_t)p * GBA_PT_D;
#pragma unroll
            for (int m = 0; m < 9; m++) PH[GP_HLL + m] = Hl[m];
#pragma unroll
            for (int m = 0; m < 3; m++) PH[GP_BL + m] = bl[m];
            maxd = fmax(fmax(fabs(Hl[0]), fabs(Hl[4])), fabs(Hl[8]));
        }
        const double chi = g2o_block_sum(S.part, chiP);
        const double md = g2o_block_max(S.part, maxd);
        if (tid == 0) { G.chiPart[blockIdx.x] = chi; G.maxPart[blockIdx.x] = md; }
        return;
    }
    // the camera half: block row r, its edges in list order
    const int r = blockIdx.x - G.ptBlocks;
    if (r >= st.nFree) return;
    const int f = G.rowKf[r], cs = G.camStart[f], ce = G.camStart[f + 1];
    const GbaCam& C = G.cams[f];
    const PoSE3 P = C.est[cur];
    const int a = (tid % 36) / 6, b = tid % 6;
    double h = 0.0;
    for (int base = cs; base < ce; base += GBA_T) {
        const int m = min(GBA_T, ce - base);
        __syncthreads();
        if (tid < m) {
            const int k = G.camEdge[base + tid];
            const GbaEdge e = G.eI[k];
            PoLin L;
            gba_linearize_edge(P, C, gba_x(G, cur, e.pt), e, robust, L);
#pragma unroll
            for (int q = 0; q < 6; q++) { S.J[tid][q] = L.Jj0[q]; S.J[tid][6 + q] = L.Jj1[q]; }
            S.J[tid][12] = L.wO; S.J[tid][13] = L.r0; S.J[tid][14] = L.r1;
        }
        __syncthreads();
        if (tid < 36) {                                                 // entry (a, b), a >= b, is g2o's upper entry (b, a)
            for (int q = 0; q < m; q++) h += (S.J[q][b] * S.J[q][12]) * S.J[q][a] + (S.J[q][6 + b] * S.J[q][12]) * S.J[q][6 + a];
        } else if (tid < 42) {
            const int c = tid - 36;
            for (int q = 0; q < m; q++) h += S.J[q][c] * S.J[q][13] + S.J[q][6 + c] * S.J[q][14];
        }
    }
    if (tid < 36) { G.Hpp[(int64_t)r * 36 + tid] = h; if (a == b) S.dg[a] = fabs(h); }
    else if (tid < 42) G.bp[r * 6 + (tid - 36)] = h;
    __syncthreads();
    if (tid == 0) G.maxPart[G.ptBlocks + r] = fmax(fmax(fmax(S.dg[0], S.dg[1]), fmax(S.dg[2], S.dg[3])), fmax(S.dg[4], S.dg[5]));
}

__global__ __launch_bounds__(GBA_T) void k_gba_begin(GbaArgs G)
{
    __shared__ double part[GBA_T / 64];
    const GbaState st = *G.st;
    if (st.stop) return;
    const int tid = threadIdx.x;
    const double chi = gba_reduce_sum(part, G.chiPart, G.ptBlocks);
    double md = 0.0;
    for (int k = tid; k < G.ptBlocks + st.nFree; k += GBA_T) md = fmax(md, G.maxPart[k]);
    md = g2o_block_max(part, md);
    if (tid) return;
    GbaState* P = G.st;
    if (!g2o_finite(chi)) { P->status = PGORB_GBA_NONFINITE; P->stop = 1; return; }
    if (st.iter == 0) g2o_lm_begin(P->lm, g2o_lm_lambda_init(md));       // computeLambdaInit over every active vertex
    P->currentChi = chi; P->iniChi = chi; P->qmax = 0;
}

struct GbaSchurShared { double D[64][12]; };

// Hschur = Hpp - sum Bi Dinv Bj' and bschur = bp - sum Bi Dinv bl (block_solver.hpp:381-439), block row r of the lower skyline
__global__ __launch_bounds__(GBA_T) void k_gba_schur(GbaArgs G, int it)
{
    __shared__ GbaSchurShared S;
    const GbaState st = *G.st;
    if (st.stop || st.iter != it) return;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= st.nFree) return;
    const double lambda = st.lm.lambda;
    const int f = G.rowKf[r], cs = G.camStart[f], ce = G.camStart[f + 1], lo = G.first[r];
    double* Row = G.A + (int64_t)G.off[r] * 36;
    for (int q = tid; q < (r - lo + 1) * 36; q += GBA_T) Row[q] = 0.0;
    __syncthreads();
    const int slot = tid / 36, ab = tid % 36, a = ab / 6, b = ab % 6;
    if (tid < 36) Row[(int64_t)(r - lo) * 36 + tid] = G.Hpp[(int64_t)r * 36 + tid] + (a == b ? lambda : 0.0);
    const bool mine = slot == 0 && b == 0;                              // these six also sum bschur's row a
    double coef = 0.0;
    for (int base = cs; base < ce; base += 64) {
        const int m = min(64, ce - base);
        __syncthreads();
        if (tid < m) {
            const int p = G.eI[G.camEdge[base + tid]].pt;
            const double* PH = G.pH + (int64_t)p * GBA_PT_D;
            double I[9];
            gba_dinv(G, p, lambda, I);
#pragma unroll
            for (int q = 0; q < 9; q++) S.D[tid][q] = I[q];
#pragma unroll
            for (int q = 0; q < 3; q++) S.D[tid][9 + q] = (I[q * 3] * PH[GP_BL] + I[q * 3 + 1] * PH[GP_BL + 1]) + I[q * 3 + 2] * PH[GP_BL + 2];
        }
        __syncthreads();
        if (slot >= 7) continue;
        for (int q = 0; q < m; q++) {
            const int ki = G.camEdge[base + q];
            const double* Wi = G.eW + (int64_t)ki * 18 + a * 3;
            const double* Di = S.D[q];
            if (mine) coef += (Wi[0] * Di[9] + Wi[1] * Di[10]) + Wi[2] * Di[11];
            const int2 rg = gba_range(G, G.eI[ki].pt);
            for (int k = rg.x; k < rg.y; k++) {
                const GbaEdge E = G.eI[k];
                const int j = E.row;
                if (E.frame < 0 || j < lo || j > r || j % 7 != slot) continue;
                const double* Wj = G.eW + (int64_t)k * 18 + b * 3;
                double v[3];
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = (Wj[0] * Di[c] + Wj[1] * Di[3 + c]) + Wj[2] * Di[6 + c];
                Row[(int64_t)(j - lo) * 36 + ab] -= (v[0] * Wi[0] + v[1] * Wi[1]) + v[2] * Wi[2];
            }
        }
    }
    if (mine) G.bs[r * 6 + a] = G.bp[r * 6 + a] - coef;
}

struct GbaSolveShared { double part[GBA_T / 64]; double panel[GBA_PANEL][36]; double diag[36]; };

__device__ __forceinline__ double* gba_blk(const GbaArgs& G, int row, int col) { return G.A + ((int64_t)G.off[row] + (col - G.first[row])) * 36; }

// L L' of the damped skyline, in place; false = a pivot is not positive (every thread returns the same)
__device__ bool gba_factor(const GbaArgs& G, GbaSolveShared& S, int n)
{
    const int tid = threadIdx.x;
    for (int kb = 0; kb < n; kb++) {
        double* D = gba_blk(G, kb, kb);
        __syncthreads();
        if (tid < 36) S.diag[tid] = D[tid];
        const int di = tid / 6, dc = tid % 6;
        for (int j = 0; j < 6; j++) {                                   // the diagonal block, one lane an entry
            __syncthreads();
            const double d = S.diag[j * 7];
            if (!(d > 0.0)) return false;
            const double rk = __dsqrt_rn(d);
            __syncthreads();
            if (tid < 36 && dc == j && di >= j) S.diag[tid] = di == j ? rk : S.diag[tid] / rk;
            __syncthreads();
            if (tid < 36 && di > j && dc > j && dc <= di) S.diag[tid] -= S.diag[di * 6 + j] * S.diag[dc * 6 + j];
        }
        __syncthreads();
        if (tid < 36) D[tid] = S.diag[tid];
        const int cs = G.colStart[kb], m = G.colStart[kb + 1] - cs;
        // the panel: row (ib, a) of column block kb, by columns
        for (int q = tid; q < m * 6; q += GBA_T) {
            const int p = q / 6, a = q % 6;
            double* Bk = gba_blk(G, G.colRows[cs + p], kb) + a * 6;
            double v[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double t = Bk[c];
#pragma unroll
                for (int k = 0; k < c; k++) t -= v[k] * S.diag[c * 6 + k];
                v[c] = t / S.diag[c * 7];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) { Bk[c] = v[c]; if (p < GBA_PANEL) S.panel[p][a * 6 + c] = v[c]; }
        }
        __syncthreads();
        // the trailing blocks (ib, jb), jb <= ib, of the rows that reach kb
        for (int64_t q = tid; q < (int64_t)m * m * 36; q += GBA_T) {
            const int pr = (int)(q / 36), w = (int)(q % 36), pa = pr / m, pb = pr % m;
            if (pb > pa) continue;                                      // colRows rises: jb <= ib
            const int ib = G.colRows[cs + pa], jb = G.colRows[cs + pb];
            const int a = w / 6, b = w % 6;
            const double* La = pa < GBA_PANEL ? &S.panel[pa][a * 6] : gba_blk(G, ib, kb) + a * 6;
            const double* Lb = pb < GBA_PANEL ? &S.panel[pb][b * 6] : gba_blk(G, jb, kb) + b * 6;
            double* Tq = gba_blk(G, ib, jb) + w;
            double t = *Tq;
#pragma unroll
            for (int k = 0; k < 6; k++) t -= La[k] * Lb[k];
            *Tq = t;
        }
    }
    __syncthreads();
    return true;
}

// L y = b by columns, then L' x = y by columns from the last; G.x holds the result
__device__ void gba_solve(const GbaArgs& G, int n)
{
    const int tid = threadIdx.x;
    for (int k = tid; k < n * 6; k += GBA_T) G.x[k] = G.bs[k];
    __syncthreads();
    for (int kb = 0; kb < n; kb++) {
        const double* D = gba_blk(G, kb, kb);
        double* y = G.x + kb * 6;
        if (tid == 0)
            for (int c = 0; c < 6; c++) {
                double t = y[c];
                for (int k = 0; k < c; k++) t -= D[c * 6 + k] * y[k];
                y[c] = t / D[c * 7];
            }
        __syncthreads();
        const int cs = G.colStart[kb], m = G.colStart[kb + 1] - cs;
        for (int q = tid; q < m * 6; q += GBA_T) {
            const int ib = G.colRows[cs + q / 6], a = q % 6;
            const double* Bk = gba_blk(G, ib, kb) + a * 6;
            double t = G.x[ib * 6 + a];
#pragma unroll
            for (int k = 0; k < 6; k++) t -= Bk[k] * y[k];
            G.x[ib * 6 + a] = t;
        }
        __syncthreads();
    }
    for (int kb = n - 1; kb >= 0; kb--) {
        const double* D = gba_blk(G, kb, kb);
        double* x = G.x + kb * 6;
        if (tid == 0)
            for (int c = 5; c >= 0; c--) {
                double t = x[c];
                for (int k = 5; k > c; k--) t -= D[k * 6 + c] * x[k];
                x[c] = t / D[c * 7];
            }
        __syncthreads();
        const int lo = G.first[kb];
        for (int q = tid; q < (kb - lo) * 6; q += GBA_T) {
            const int jb = lo + q / 6, b = q % 6;
            const double* Bk = gba_blk(G, kb, jb);
            double t = G.x[jb * 6 + b];
#pragma unroll
            for (int k = 5; k >= 0; k--) t -= Bk[k * 6 + b] * x[k];
            G.x[jb * 6 + b] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GBA_T) void k_gba_solve(GbaArgs G, int it)
{
    __shared__ GbaSolveShared S;
    const GbaState st = *G.st;
    if (st.stop || st.iter != it) return;
    const int tid = threadIdx.x, n = st.nFree, cur = st.cur;
    const bool ok2 = gba_factor(G, S, n);
    __syncthreads();
    if (ok2) gba_solve(G, n);
    else
        for (int k = tid; k < n * 6; k += GBA_T) G.x[k] = 0.0;          // a failed factorisation: the trial stays at the estimates
    __syncthreads();
    // update() of the cameras, and computeScale's camera rows
    for (int r = tid; r < n; r += GBA_T) {
        GbaCam& C = G.cams[G.rowKf[r]];
        const double u[6] = {G.x[r * 6], G.x[r * 6 + 1], G.x[r * 6 + 2], G.x[r * 6 + 3], G.x[r * 6 + 4], G.x[r * 6 + 5]};
        C.est[cur ^ 1] = ok2 ? po_oplus(C.est[cur], u) : C.est[cur];
    }
    double sc = 0.0;
    for (int k = tid; k < n * 6; k += GBA_T) sc += G.x[k] * (st.lm.lambda * G.x[k] + G.bp[k]);
    sc = g2o_block_sum(S.part, sc);
    if (tid == 0) { G.st->ok2 = ok2 ? 1 : 0; G.st->camScale = sc; }
}

// xl = Dinv * (bl - B' xp) (block_solver.hpp:459-483), update() of the points, activeRobustChi2 at the trial, computeScale's point terms
__global__ __launch_bounds__(GBA_T) void k_gba_try(GbaArgs G, int it)
{
    __shared__ double part[GBA_T / 64];
    const GbaState st = *G.st;
    if (st.stop || st.iter != it) return;
    const int tid = threadIdx.x, cur = st.cur, p = blockIdx.x * GBA_T + tid;
    const bool robust = G.robust != 0, ok2 = st.ok2 != 0;
    const double lambda = st.lm.lambda;
    double chiP = 0.0, sc = 0.0;
    if (p < G.npoints && G.pInc[p]) {
        const double* PH = G.pH + (int64_t)p * GBA_PT_D;
        const int2 rg = gba_range(G, p);
        double xl[3] = {0.0, 0.0, 0.0};
        if (ok2) {
            double I[9], cl[3] = {PH[GP_BL], PH[GP_BL + 1], PH[GP_BL + 2]};
            gba_dinv(G, p, lambda, I);
            for (int k = rg.x; k < rg.y; k++) {
                const GbaEdge e = G.eI[k];
                if (e.frame < 0 || e.row < 0) continue;
                const double* Wb = G.eW + (int64_t)k * 18;
                const double* xp = G.x + e.row * 6;
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < 6; a++) s += Wb[a * 3 + m] * xp[a];
                    cl[m] -= s;
                }
            }
#pragma unroll
            for (int m = 0; m < 3; m++) xl[m] = (I[m * 3] * cl[0] + I[m * 3 + 1] * cl[1]) + I[m * 3 + 2] * cl[2];
        }
        const double* X = gba_x(G, cur, p);
        double* Xt = gba_x(G, cur ^ 1, p);
        double xt[3];
#pragma unroll
        for (int m = 0; m < 3; m++) { xt[m] = X[m] + xl[m]; Xt[m] = xt[m]; }
        sc = (xl[0] * (lambda * xl[0] + PH[GP_BL]) + xl[1] * (lambda * xl[1] + PH[GP_BL + 1])) + xl[2] * (lambda * xl[2] + PH[GP_BL + 2]);
        for (int k = rg.x; k < rg.y; k++) {
            const GbaEdge e = G.eI[k];
            if (e.frame < 0) continue;
            const GbaCam& C = G.cams[e.frame];
            double e0, e1;
            gba_error(C.est[e.row >= 0 ? cur ^ 1 : cur], C, xt, e, e0, e1);
            double c2 = g2o_chi2(e0, e1, (double)e.w), r0 = c2, r1;
            if (robust) g2o_huber(c2, GBA_DELTA, r0, r1);
            chiP += r0;
        }
    }
    const double chi = g2o_block_sum(part, chiP);
    const double scs = g2o_block_sum(part, sc);
    if (tid == 0) { G.chiPart[blockIdx.x] = chi; G.scPart[blockIdx.x] = scs; }
}

// rho, accept or reject, lambda and nu (optimization_algorithm_levenberg.cpp:110-150); at the end of the trial loop the stop rules
__global__ __launch_bounds__(GBA_T) void k_gba_decide(GbaArgs G, int it)
{
    __shared__ double part[GBA_T / 64];
    GbaState st = *G.st;
    if (st.stop || st.iter != it) return;
    const double tempChi = gba_reduce_sum(part, G.chiPart, G.ptBlocks);
    const double scale = st.camScale + gba_reduce_sum(part, G.scPart, G.ptBlocks);
    if (threadIdx.x) return;
    double rho;
    if (g2o_lm_decide(st.lm, st.currentChi, tempChi, st.ok2 != 0, scale, rho)) st.cur ^= 1;      // discardTop: the trial estimates are the estimates; else pop
    st.qmax++; st.trials++;
    if (!g2o_lm_again(rho, st.qmax)) {
        const bool stop = g2o_lm_stop(st.lm, st.iniChi, st.currentChi, st.qmax, rho);
        st.its++; st.iter++;
        if (stop || st.iter >= G.iterations) st.stop = 1;
    }
    *G.st = st;
}

// Recover optimized data (:186-236)
__global__ __launch_bounds__(GBA_T) void k_gba_finish(GbaArgs G)
{
    const GbaState st = *G.st;
    const int64_t g = (int64_t)blockIdx.x * GBA_T + threadIdx.x;
    const bool keepIn = st.status != 0;
    const int cur = keepIn ? 0 : st.cur;
    if (g < G.nkf) {
        const int f = (int)g;
        pgorb_kf_pose o = G.pose[f];
        const bool live = !gba_bad(G, f);
        if (live) {
            // Converter::toCvMat(vSE3->estimate()), then SetPose's Ow = -Rcw.t()*tcw; under a status the estimate is toSE3Quat(pose)
            const PoSE3 E = keepIn ? po_from_pose(o) : G.cams[f].est[cur];
            po_set_pose(E, o);
        }
        G.poseOut[f] = o;
        G.kfDone[f] = live ? 1 : 0;
    }
    if (g < G.npoints) {
        const int p = (int)g;
        const bool done = G.pInc[p] != 0;
        float pos[3] = {G.pts[p].pos[0], G.pts[p].pos[1], G.pts[p].pos[2]};
        if (done && !keepIn) {
            const double* X = gba_x(G, cur, p);
#pragma unroll
            for (int m = 0; m < 3; m++) pos[m] = __double2float_rn(X[m]);
            if (G.inPlace) { G.pts[p].pos[0] = pos[0]; G.pts[p].pos[1] = pos[1]; G.pts[p].pos[2] = pos[2]; }
        }
        G.posOut[(int64_t)p * 3] = pos[0]; G.posOut[(int64_t)p * 3 + 1] = pos[1]; G.posOut[(int64_t)p * 3 + 2] = pos[2];
        G.ptDone[p] = done ? 1 : 0;
    }
    if (G.chi2 && g < G.nobs) {
        float c2 = 0.0f;
        const GbaEdge e = G.eI[g];
        if (!keepIn && e.frame >= 0) {
            const GbaCam& C = G.cams[e.frame];
            double e0, e1;
            gba_error(C.est[cur], C, gba_x(G, cur, e.pt), e, e0, e1);
            c2 = __double2float_rn(g2o_chi2(e0, e1, (double)e.w));
        }
        G.chi2[g] = c2;
    }
    if (g == 0 && G.info) {
        const bool nf = st.status == PGORB_GBA_NONFINITE;
        int32_t* I = G.info;
        I[0] = st.status; I[1] = st.nE; I[2] = st.nPts; I[3] = st.nVert; I[4] = keepIn ? 0 : st.nFree;
        I[5] = (keepIn || nf) ? 0 : st.its; I[6] = (keepIn || nf) ? 0 : st.trials; I[7] = st.env;
    }
}

extern "C" {

int pgorb_global_bundle_adjustment_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap,
        const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, const uint8_t* d_kf_fixed_id0,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        const int32_t* d_obs_idx, int nobs, int iterations, int robust, int in_place,
        pgorb_kf_pose* d_pose_out, float* d_pos_out, uint8_t* d_kf_done, uint8_t* d_point_done, float* d_chi2, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || iterations < 0 || !d_info || !d_obs_start ||
        (nframes && (!d_kps || !d_n || !d_pose || !d_pose_out || !d_kf_done || d_pose_out == d_pose)) ||
        (npoints && (!d_points || !d_pos_out || !d_point_done)) || (nobs && (!d_obs_frame || !d_obs_idx)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_global_bundle_adjustment_device");
    if (cap > GBA_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than 16000 keypoints per frame");
    if (nframes > PGORB_GBA_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_KF key frames");
    if (npoints > PGORB_GBA_MAX_POINTS) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_POINTS points");
    if (nobs > PGORB_GBA_MAX_EDGES) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_EDGES observations");
    GbaArgs G;
    memset(&G, 0, sizeof(G));
    G.nlevels = pgorb_levels(c);
    if (!(G.nlevels > 0) || G.nlevels > PG_MAXL || pgorb_scale_tables(c, nullptr, nullptr, nullptr, G.invSigma2) < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    G.K = d_kps; G.n = d_n; G.cap = cap; G.nkf = nframes; G.pose = d_pose; G.kfBad = d_kf_bad; G.id0 = d_kf_fixed_id0;
    G.npoints = npoints; G.pts = d_points; G.ptBad = d_point_bad; G.obsStart = d_obs_start; G.obsFrame = d_obs_frame; G.obsIdx = d_obs_idx; G.nobs = nobs;
    G.iterations = iterations; G.robust = robust ? 1 : 0; G.inPlace = in_place ? 1 : 0;
    G.poseOut = d_pose_out; G.posOut = d_pos_out; G.kfDone = d_kf_done; G.ptDone = d_point_done; G.chi2 = d_chi2; G.info = d_info;
    G.envCap = (int)std::min<int64_t>(PGORB_GBA_MAX_ENVELOPE_BLOCKS, (int64_t)nframes * (nframes + 1) / 2);
    G.ptBlocks = (npoints + GBA_T - 1) / GBA_T;
    // the arena: 8-byte items first
    const size_t K = (size_t)std::max(nframes, 1), Np = (size_t)std::max(npoints, 1), No = (size_t)std::max(nobs, 1), V = (size_t)std::max(G.envCap, 1),
                 Pb = (size_t)std::max(G.ptBlocks, 1);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t oSt = take(sizeof(GbaState)), oCams = take(K * sizeof(GbaCam)), oEW = take(No * 18 * 8), oPX = take(Np * 6 * 8), oPH = take(Np * GBA_PT_D * 8),
                 oHpp = take(K * 36 * 8), oBp = take(K * 6 * 8), oBs = take(K * 6 * 8), oX = take(K * 6 * 8), oA = take(V * 36 * 8),
                 oChi = take(Pb * 8), oMax = take((Pb + K) * 8), oSc = take(Pb * 8), oEI = take(No * sizeof(GbaEdge)), oInc = take(Np * 4),
                 oSys = take(K * 4), oRowKf = take(K * 4), oCamStart = take((K + 1) * 4), oCamEdge = take(No * 4),
                 oChunk = take(K * GBA_CHUNKS * 4), oTmp = take((K + 1) * 4), oFirst = take(K * 4), oOff = take((K + 1) * 4),
                 oColStart = take((K + 1) * 4), oColRows = take(V * 4);
    void* scr;
    int rc = pg_ctx_scratch(c, at, s, &scr);
    if (rc) return rc;
    uint8_t* p = (uint8_t*)scr;
    G.st = (GbaState*)(p + oSt); G.cams = (GbaCam*)(p + oCams); G.eW = (double*)(p + oEW); G.pX = (double*)(p + oPX); G.pH = (double*)(p + oPH);
    G.Hpp = (double*)(p + oHpp); G.bp = (double*)(p + oBp); G.bs = (double*)(p + oBs); G.x = (double*)(p + oX); G.A = (double*)(p + oA);
    G.chiPart = (double*)(p + oChi); G.maxPart = (double*)(p + oMax); G.scPart = (double*)(p + oSc); G.eI = (GbaEdge*)(p + oEI);
    G.pInc = (int32_t*)(p + oInc); G.sys = (int32_t*)(p + oSys); G.rowKf = (int32_t*)(p + oRowKf); G.camStart = (int32_t*)(p + oCamStart);
    G.camEdge = (int32_t*)(p + oCamEdge); G.chunkCnt = (int32_t*)(p + oChunk); G.tmp = (int32_t*)(p + oTmp); G.first = (int32_t*)(p + oFirst);
    G.off = (int32_t*)(p + oOff); G.colStart = (int32_t*)(p + oColStart); G.colRows = (int32_t*)(p + oColRows);
    hipLaunchKernelGGL(k_gba_prepare, dim3(1), dim3(GBA_PREP_T), 0, s, G);
    if (nframes > 0 && npoints > 0 && nobs > 0)
        for (int it = 0; it < iterations; it++) {
            hipLaunchKernelGGL(k_gba_linearize, dim3((unsigned)(G.ptBlocks + nframes)), dim3(GBA_T), 0, s, G);
            hipLaunchKernelGGL(k_gba_begin, dim3(1), dim3(GBA_T), 0, s, G);
            for (int q = 0; q < G2O_LM_TRIALS; q++) {
                hipLaunchKernelGGL(k_gba_schur, dim3((unsigned)nframes), dim3(GBA_T), 0, s, G, it);
                hipLaunchKernelGGL(k_gba_solve, dim3(1), dim3(GBA_T), 0, s, G, it);
                hipLaunchKernelGGL(k_gba_try, dim3((unsigned)G.ptBlocks), dim3(GBA_T), 0, s, G, it);
                hipLaunchKernelGGL(k_gba_decide, dim3(1), dim3(GBA_T), 0, s, G, it);
            }
        }
    const int64_t items = std::max<int64_t>(std::max<int64_t>(nframes, npoints), std::max<int64_t>(nobs, 1));
    hipLaunchKernelGGL(k_gba_finish, dim3((unsigned)((items + GBA_T - 1) / GBA_T)), dim3(GBA_T), 0, s, G);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "a global-bundle-adjustment launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool gba_all_finite(const float* v, int n)
{
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

// host buffers: the device form over one staged copy; the inputs are checked here
int pgorb_global_bundle_adjustment(pgorb_ctx* c, int nkf, const pgorb_keypoint* const* kps, const int32_t* n, const pgorb_kf_pose* pose,
        const uint8_t* kf_bad, const uint8_t* kf_fixed_id0, int npoints, pgorb_map_point* points, const uint8_t* point_bad,
        const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx, int iterations, int robust, int in_place,
        pgorb_kf_pose* pose_out, float* pos_out, uint8_t* kf_done, uint8_t* point_done, float* chi2, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    const int nlevels = pgorb_levels(c);
    int cap = 1, nobs = 0;
    if (nkf < 0 || npoints < 0) why = "a count is negative";
    else if (iterations < 0) why = "iterations is negative";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_global_bundle_adjustment: ") + why).c_str());
    if (nkf > PGORB_GBA_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_KF key frames");
    if (npoints > PGORB_GBA_MAX_POINTS) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_POINTS points");
    if (!obs_start || (nkf && (!kps || !n || !pose || !pose_out || !kf_done)) || (npoints && (!points || !pos_out || !point_done)))
        why = "an array that is read or written is NULL";
    for (int f = 0; !why && f < nkf; f++) {
        if (n[f] < 0 || (n[f] && !kps[f])) why = "a key frame's count is negative or its keypoints are NULL";
        else if (!gba_all_finite(pose[f].Tcw, 12) || !gba_all_finite(&pose[f].fx, 4)) why = "a pose or a camera is not finite";
        else if (pose[f].fx == 0.0f || pose[f].fy == 0.0f) why = "fx or fy is zero";
        else cap = std::max(cap, n[f]);
    }
    if (!why && obs_start[0] != 0) why = "obs_start[0] must be 0";
    for (int p = 0; !why && p < npoints; p++) {
        if (obs_start[p + 1] < obs_start[p]) why = "obs_start decreases";
        else if (!gba_all_finite(points[p].pos, 3)) why = "a point is not finite";
    }
    if (!why) {
        nobs = obs_start[npoints];
        if (nobs && (!obs_frame || !obs_idx)) why = "an array that is read or written is NULL";
    }
    if (!why && nobs > PGORB_GBA_MAX_EDGES)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than PGORB_GBA_MAX_EDGES observations");
    std::vector<int32_t> seen((size_t)std::max(nkf, 1), -1);
    for (int p = 0; !why && p < npoints; p++)
        for (int k = obs_start[p]; !why && k < obs_start[p + 1]; k++) {
            const int f = obs_frame[k];
            if (f < 0 || f >= nkf || obs_idx[k] < 0 || obs_idx[k] >= n[f]) why = "an observation names a key frame or keypoint out of range";
            else if (seen[f] == p) why = "a list names a key frame twice";
            else if (kps[f][obs_idx[k]].octave < 0 || kps[f][obs_idx[k]].octave >= nlevels) why = "an octave is outside the context's levels";
            else seen[f] = p;
        }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_global_bundle_adjustment: ") + why).c_str());
    for (int f = 0; f < nkf; f++)
        if (n[f] > GBA_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: more than 16000 keypoints per frame");
    const int nf = std::max(nkf, 1), np = std::max(npoints, 1), no = std::max(nobs, 1);
    const size_t kb = sizeof(pgorb_keypoint);
    PgHostCall s(c);
    const size_t oK = s.region(PG_UP, (size_t)nf * cap * kb), oN = s.region(PG_UP, (size_t)nf * 4), oPose = s.region(PG_UP, (size_t)nf * sizeof(pgorb_kf_pose)),
                 oKB = s.region(PG_UP, nf), oId = s.region(PG_UP, nf), oB = s.region(PG_UP, np), oOS = s.region(PG_UP, (size_t)(npoints + 1) * 4),
                 oOF = s.region(PG_UP, (size_t)no * 4), oOI = s.region(PG_UP, (size_t)no * 4),
                 oP = s.region(PG_INOUT, (size_t)np * sizeof(pgorb_map_point)),
                 oPO = s.region(PG_DOWN, (size_t)nf * sizeof(pgorb_kf_pose)), oXO = s.region(PG_DOWN, (size_t)np * 12), oKD = s.region(PG_DOWN, nf),
                 oPD = s.region(PG_DOWN, np), oChi = s.region(PG_DOWN, (size_t)no * 4), oR = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    for (int f = 0; f < nkf; f++) s.put(oK, kps[f], (size_t)n[f] * kb, (size_t)f * cap * kb, (size_t)cap * kb);
    s.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    s.put(oPose, pose, (size_t)nkf * sizeof(pgorb_kf_pose), 0, (size_t)nf * sizeof(pgorb_kf_pose));
    s.put(oKB, kf_bad, nkf, 0, nf);
    s.put(oId, kf_fixed_id0, nkf, 0, nf);
    s.put(oB, point_bad, npoints, 0, np);
    s.put(oOS, obs_start, (size_t)(npoints + 1) * 4);
    s.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    s.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    s.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    if ((rc = s.run([&] {
            return pgorb_global_bundle_adjustment_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), nkf, cap, s.dev<pgorb_kf_pose>(oPose),
                    s.dev(oKB), s.dev(oId), npoints, s.dev<pgorb_map_point>(oP), s.dev(oB), s.dev<int32_t>(oOS), s.dev<int32_t>(oOF),
                    s.dev<int32_t>(oOI), nobs, iterations, robust, in_place, s.dev<pgorb_kf_pose>(oPO), s.dev<float>(oXO), s.dev(oKD), s.dev(oPD),
                    chi2 ? s.dev<float>(oChi) : nullptr, s.dev<int32_t>(oR), nullptr); }))) return rc;
    if (in_place) memcpy(points, s.host(oP), (size_t)npoints * sizeof(pgorb_map_point));
    memcpy(pose_out, s.host(oPO), (size_t)nkf * sizeof(pgorb_kf_pose));
    if (npoints) { memcpy(pos_out, s.host(oXO), (size_t)npoints * 12); memcpy(point_done, s.host(oPD), npoints); }
    if (nkf) memcpy(kf_done, s.host(oKD), nkf);
    if (chi2 && nobs) memcpy(chi2, s.host(oChi), (size_t)nobs * 4);
    const int32_t* r = s.host<int32_t>(oR);
    if (info) memcpy(info, r, PGORB_GBA_INFO * 4);
    if (r[0] & PGORB_GBA_LIMIT)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_global_bundle_adjustment: the envelope exceeds PGORB_GBA_MAX_ENVELOPE_BLOCKS");
    return r[4];
}

}  // extern "C"
