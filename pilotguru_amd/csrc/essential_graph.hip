// essential_graph.hip -- Optimizer::OptimizeEssentialGraph on gfx950: loop closing's Sim3 pose graph over the whole map, ONE problem
// spread over many workgroups and a fixed sequence of launches on the caller's stream.
//
// Restates (thirdparty/orb-slam2, thirdparty/g2o):
//   Optimizer::OptimizeEssentialGraph             src/Optimizer.cc:781-1044
//   Sim3 (operator*, inverse, map, Sim3(Vector7d), log)   g2o/types/sim3.h (g2o_sim3.h)
//   VertexSim3Expmap::oplusImpl, EdgeSim3::computeError   g2o/types/types_seven_dof_expmap.h:60-88, :99-114
//   BaseBinaryEdge::linearizeOplus                g2o/core/base_binary_edge.hpp:131-205 (central differences, delta = 1e-9, fixed vertices skipped)
//   BaseBinaryEdge::constructQuadraticForm        :55-90 (information = identity, no robust kernel)
//   BlockSolver<7, 3>::buildSystem / solve        g2o/core/block_solver.hpp (nothing is marginalised: no Schur complement)
//   OptimizationAlgorithmLevenberg::solve         g2o/core/optimization_algorithm_levenberg.cpp:61-165 (setUserLambdaInit(1e-16))
// in double, under the readings of DESIGN.md section 4 (the OptimizeEssentialGraph rows).  LinearSolverEigen's SimplicialLDLT with a
// fill-reducing ordering is READ as a Cholesky L L' in index order; it is stored as a block skyline (row i keeps its 7 x 7 blocks from
// its lowest connected neighbour to i; fill never leaves that envelope), and every entry receives its products in the order of the
// dense index-order factorisation, so skipping the structural zeros changes no bit.  Levenberg's step control, the block reduction and
// the finite test are g2o_lm.h's single copies (shared with pose_opt.hip, optimize_sim3.hip, local_ba.hip, global_ba.hip); Sim3 is
// g2o_sim3.h's (shared with optimize_sim3.hip and loop_pose.h).
//
// Launches (no host round trip, no cooperative launch, no wait between workgroups; every loop is bounded by a capacity or a constant):
//   k_eg_prepare    one workgroup: the vertices, the filtered candidates with their ranks (= the edge order), the measurements, the
//                   per-vertex incident-edge lists in edge order, the system indices, the envelope and its column lists in row order.
//   k_eg_linearize  all CUs, one work item per (edge, side, column): the two perturbed errors and the Jacobian column, in LDS; then
//                   per edge the blocks Ji'Ji, Ji'Jj, Jj'Jj and the vectors -Ji'e, -Jj'e.
//   k_eg_assemble   all CUs, one workgroup per block row: lane (a, b) adds entry (a, b) of the row's incident edges in edge order
//                   into the diagonal and off-diagonal blocks of the skyline -- one owner per entry, no atomics.
//   k_eg_step       one workgroup: the chi2 the iteration starts from, then Levenberg's trial loop (at most 10): damp, factor (the
//                   panel of the pivot column staged in LDS), solve, oplus into trial estimates, the chi2 of all edges and
//                   computeScale in one fixed tree, rho, accept or reject; then the stop rules, left in the graph's state.
//   k_eg_finish     all CUs: pose_out, sim3_out, edge_out, the point correction, info.
// The three kernels of an iteration return at once when the state's stop flag is set.
#include "kf_window.h"
#include "loop_pose.h"                     // lp_map, lp_pose_from_sim3: shared with loop_correct.hip
#include <math.h>
#include <string>

#define EG_T 256                  // k_eg_step
#define EG_PREP_T 1024
#define EG_LIN_EDGES 16
#define EG_LIN_T (EG_LIN_EDGES * 14)
#define EG_PANEL 64               // blocks of a pivot column kept in LDS
// per edge doubles: the error, chi2, b of both sides, the three blocks (169, kept at an even count)
#define ED_ERR 0
#define ED_CHI 7
#define ED_BI 8
#define ED_BJ 15
#define ED_HII 22
#define ED_HIJ 71
#define ED_HJJ 120
#define EG_ED 170

struct EgEdge { int32_t v0, v1, kind, pad; OsSim C; };
static_assert(sizeof(EgEdge) == 80 && sizeof(OsSim) == sizeof(pgorb_sim3d), "the edge record; pgorb_sim3d is g2o::Sim3's r, t, s");

struct EgState { int32_t status, stop, nVert, nFree, nEdges, nKind[4], its, trials, env, iter, pad; G2oLm lm; };

struct EgArgs {
    int nkf; const uint64_t* id; const pgorb_kf_pose* pose; const uint8_t* bad; int loopKf, curKf, fixScale;
    const uint8_t* hasCor; const OsSim* cor; const uint8_t* hasNon; const OsSim* non;
    int nlc; const int32_t* lc; const int32_t* parent; const int32_t* leStart; const int32_t* le; int nle;
    const int32_t* cvStart; const int32_t* cv; const int32_t* cvW; int ncv; int minFeat, iterations;
    int npoints; pgorb_map_point* pts; const uint8_t* pbad; const int32_t* pref;
    pgorb_sim3d* simOut; pgorb_kf_pose* poseOut; pgorb_eg_edge* edgeOut; int32_t* info;
    // the arena
    int ncand, envCap;
    EgState* st; OsSim* est; OsSim* trial; OsSim* scw;
    int32_t* sys; int32_t* rowKf; int32_t* deg; int32_t* incStart; int32_t* incEdge; int32_t* cursor;
    int32_t* keep; int32_t* rank; EgEdge* edges; double* ed;
    int32_t* first; int32_t* off; int32_t* colStart; int32_t* colRows;
    double* A; double* L; double* b; double* x;
};

__device__ __forceinline__ bool eg_bad(const EgArgs& G, int i) { return G.bad && G.bad[i]; }
__device__ __forceinline__ bool eg_kf(const EgArgs& G, int i) { return i >= 0 && i < G.nkf && !eg_bad(G, i); }

// EdgeSim3::computeError: (C * v1 * v2^-1).log()
__device__ __forceinline__ void eg_error(const OsSim& C, const OsSim& Si, const OsSim& Sj, double (&e)[7])
{
    os_log(os_mul(os_mul(C, Si), os_inverse(Sj)), e);
}
// chi2 = _error.dot(information * _error), information = identity
__device__ __forceinline__ double eg_chi2(const double (&e)[7])
{
    double c = 0.0;
#pragma unroll
    for (int r = 0; r < 7; r++) c += e[r] * e[r];
    return c;
}

// the per-key-frame clamp of a CSR row whose start array nobody checked
__device__ __forceinline__ int2 eg_row(const int32_t* start, int i, int n)
{
    const int a = min(max(start[i], 0), n), b = min(max(start[i + 1], 0), n);
    return make_int2(a, max(a, b));
}

// exclusive scan of in[0 .. n) into out (may be in), every thread of the workgroup calls it; returns the total
__device__ int eg_scan(const int32_t* in, int32_t* out, int n, int32_t* part /* LDS [T + 1] */)
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

// NonCorrectedSim3 where present, else vScw
__device__ __forceinline__ OsSim eg_non_corrected(const EgArgs& G, int i) { return (G.hasNon && G.hasNon[i]) ? G.non[i] : G.scw[i]; }

// The candidates of key frame i after its own parent candidate: calls f(candidate index, other key frame, kind, kept)
template <class F>
__device__ __forceinline__ void eg_walk(const EgArgs& G, int i, F&& f)
{
    const int2 lr = eg_row(G.leStart, i, G.nle), cr = eg_row(G.cvStart, i, G.ncv);
    const int base = G.nlc + i + lr.x + cr.x;
    const bool live = !eg_bad(G, i);
    const int p = G.parent[i];
    f(base, p, 1, live && p != i && eg_kf(G, p));                                    // the spanning-tree edge (:901-923)
    for (int k = lr.x; k < lr.y; k++) {                                              // pLKF->mnId < pKF->mnId (:930)
        const int l = G.le[k];
        f(base + 1 + (k - lr.x), l, 2, live && l != i && eg_kf(G, l) && G.id[l] < G.id[i]);
    }
    const int cb = base + 1 + (lr.y - lr.x);
    for (int k = cr.x; k < cr.y; k++) {                                              // :952-982
        const int n = G.cv[k];
        bool ok = live && n != i && eg_kf(G, n) && G.cvW[k] >= G.minFeat && n != p && G.parent[n] != i && G.id[n] < G.id[i];
        for (int q = lr.x; ok && q < lr.y; q++) ok = G.le[q] != n;                   // !sLoopEdges.count(pKFn)
        for (int c = 0; ok && c < G.nlc; c++)                                        // sInsertedEdges (:878, :960)
            if (G.keep[c]) {
                const int a = G.lc[c * 3], b = G.lc[c * 3 + 1];
                ok = !((a == i && b == n) || (a == n && b == i));
            }
        f(cb + (k - cr.x), n, 3, ok);
    }
}

__global__ __launch_bounds__(EG_PREP_T) void k_eg_prepare(EgArgs G)
{
    __shared__ int32_t part[EG_PREP_T + 1];
    __shared__ int32_t kinds[4];
    const int tid = threadIdx.x, nkf = G.nkf;
    if (tid < 4) kinds[tid] = 0;
    // the vertices (:809-844) and the loop connections' filter (:863)
    for (int i = tid; i < nkf; i += EG_PREP_T) {
        OsSim S;
        if (G.hasCor && G.hasCor[i]) S = G.cor[i];
        else S = lp_sim3_from_pose(G.pose[i].Tcw);
        G.scw[i] = S; G.est[i] = S; G.trial[i] = S;
        G.sys[i] = -1; G.deg[i] = 0; G.cursor[i] = 0;
    }
    for (int c = tid; c < G.nlc; c += EG_PREP_T) {
        const int i = G.lc[c * 3], j = G.lc[c * 3 + 1], w = G.lc[c * 3 + 2];
        G.keep[c] = (eg_kf(G, i) && eg_kf(G, j) && i != j && ((i == G.curKf && j == G.loopKf) || w >= G.minFeat)) ? 1 : 0;
    }
    for (int c = G.nlc + tid; c < G.ncand; c += EG_PREP_T) G.keep[c] = 0;
    __syncthreads();
    for (int i = tid; i < nkf; i += EG_PREP_T) eg_walk(G, i, [&](int c, int, int, bool kept) { if (kept) G.keep[c] = 1; });
    __syncthreads();
    const int nE = eg_scan(G.keep, G.rank, G.ncand, part);
    // the edges at their ranks, with their measurements
    for (int c = tid; c < G.nlc; c += EG_PREP_T)
        if (G.keep[c]) {
            EgEdge E;
            E.v0 = G.lc[c * 3]; E.v1 = G.lc[c * 3 + 1]; E.kind = 0; E.pad = 0;
            E.C = os_mul(G.scw[E.v1], os_inverse(G.scw[E.v0]));                      // Sji = Sjw * Swi (:857-867)
            G.edges[G.rank[c]] = E;
            atomicAdd(&kinds[0], 1);
        }
    for (int i = tid; i < nkf; i += EG_PREP_T) {
        if (eg_bad(G, i)) continue;
        const OsSim Swi = os_inverse(eg_non_corrected(G, i));                        // :889-896
        eg_walk(G, i, [&](int c, int j, int kind, bool kept) {
            if (!kept || !G.keep[c]) return;
            EgEdge E;
            E.v0 = i; E.v1 = j; E.kind = kind; E.pad = 0;
            E.C = os_mul(eg_non_corrected(G, j), Swi);
            G.edges[G.rank[c]] = E;
            atomicAdd(&kinds[kind], 1);
        });
    }
    __syncthreads();
    // the incident-edge lists: integer counters give the degrees (a count has no order); then a vertex's thread walks the edges in edge
    // order and writes its own list, so the list is in edge order by construction (nkf x edges reads over 1024 threads, all lanes on
    // the same edge at once)
    for (int e = tid; e < nE; e += EG_PREP_T) { atomicAdd(&G.deg[G.edges[e].v0], 1); atomicAdd(&G.deg[G.edges[e].v1], 1); }
    __syncthreads();
    eg_scan(G.deg, G.incStart, nkf, part);
    if (tid == 0) G.incStart[nkf] = 2 * nE;
    __syncthreads();
    for (int i = tid; i < nkf; i += EG_PREP_T) {
        const int d = G.deg[i];
        int32_t* Lst = G.incEdge + G.incStart[i];
        int at = 0;
        for (int e = 0; e < nE && at < d; e++) {
            const EgEdge& E = G.edges[e];
            if (E.v0 == i || E.v1 == i) Lst[at++] = e;
        }
        G.cursor[i] = (d > 0 && i != G.loopKf) ? 1 : 0;                              // free: active and not fixed (:834)
    }
    __syncthreads();
    const int nFree = eg_scan(G.cursor, G.sys, nkf, part);
    for (int i = tid; i < nkf; i += EG_PREP_T) {
        if (G.cursor[i]) G.rowKf[G.sys[i]] = i; else G.sys[i] = -1;
    }
    __syncthreads();
    // the envelope: row r reaches down to its lowest free neighbour
    for (int r = tid; r < nFree; r += EG_PREP_T) {
        const int v = G.rowKf[r];
        int lo = r;
        for (int k = G.incStart[v]; k < G.incStart[v + 1]; k++) {
            const EgEdge& E = G.edges[G.incEdge[k]];
            const int u = G.sys[E.v0 == v ? E.v1 : E.v0];
            if (u >= 0) lo = min(lo, u);
        }
        G.first[r] = lo;
        G.cursor[r] = r - lo + 1;
    }
    __syncthreads();
    const int env = eg_scan(G.cursor, G.off, nFree, part);
    if (tid == 0) G.off[nFree] = env;
    const bool fits = env <= G.envCap;
    // the rows below the diagonal that reach column k, in increasing row: a column's thread counts them, then writes them
    for (int k = tid; k < nFree; k += EG_PREP_T) {
        int m = 0;
        if (fits)
            for (int r = k + 1; r < nFree; r++) m += G.first[r] <= k ? 1 : 0;
        G.cursor[k] = m;
    }
    __syncthreads();
    eg_scan(G.cursor, G.colStart, nFree, part);
    if (tid == 0) G.colStart[nFree] = fits ? env - nFree : 0;
    if (fits)
        for (int k = tid; k < nFree; k += EG_PREP_T) {
            int at = G.colStart[k];
            for (int r = k + 1; r < nFree; r++)
                if (G.first[r] <= k) G.colRows[at++] = r;
        }
    if (tid == 0) {
        EgState S;
        memset(&S, 0, sizeof(S));
        int nv = 0;
        for (int i = 0; i < nkf; i++) nv += eg_bad(G, i) ? 0 : 1;
        S.nVert = nv; S.nFree = nFree; S.nEdges = nE; S.env = env;
        for (int k = 0; k < 4; k++) S.nKind[k] = kinds[k];
        if (nE == 0 || nFree == 0) S.status = PGORB_EG_NOTHING;
        else if (!fits) S.status = PGORB_EG_LIMIT;
        S.stop = (S.status || G.iterations <= 0) ? 1 : 0;
        S.lm.ni = 2;
        *G.st = S;
    }
}

struct EgLinShared { double J[EG_LIN_EDGES][2][49]; double err[EG_LIN_EDGES][7]; };

__global__ __launch_bounds__(EG_LIN_T) void k_eg_linearize(EgArgs G)
{
    __shared__ EgLinShared S;
    if (G.st->stop) return;
    const int nE = G.st->nEdges, tid = threadIdx.x;
    const int le = tid / 14, item = tid % 14, side = item / 7, d = item % 7;
    const int e = blockIdx.x * EG_LIN_EDGES + le;
    bool fixedI = true, fixedJ = true;
    if (e < nE) {
        const EgEdge E = G.edges[e];
        const OsSim Si = G.est[E.v0], Sj = G.est[E.v1];
        fixedI = E.v0 == G.loopKf; fixedJ = E.v1 == G.loopKf;
        double col[7];
#pragma unroll
        for (int r = 0; r < 7; r++) col[r] = 0.0;
        if (!(side ? fixedJ : fixedI)) {
            // linearizeOplus: push, oplus(+delta e_d), computeError, pop; the same at -delta; under _fix_scale oplusImpl zeroes update[6]
            const double scalar = 1.0 / (2.0 * 1e-9);
            double ep[7], em[7], u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == d ? 1e-9 : 0.0;
            if (G.fixScale) u[6] = 0.0;
            const OsSim Sp = os_mul(os_exp(u), side ? Sj : Si);
            if (side) eg_error(E.C, Si, Sp, ep); else eg_error(E.C, Sp, Sj, ep);
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = k == d ? -1e-9 : 0.0;
            if (G.fixScale) u[6] = 0.0;
            const OsSim Sm = os_mul(os_exp(u), side ? Sj : Si);
            if (side) eg_error(E.C, Si, Sm, em); else eg_error(E.C, Sm, Sj, em);
#pragma unroll
            for (int r = 0; r < 7; r++) col[r] = scalar * (ep[r] - em[r]);
        }
#pragma unroll
        for (int r = 0; r < 7; r++) S.J[le][side][r * 7 + d] = col[r];
        if (item == 0) {
            double er[7];
            eg_error(E.C, Si, Sj, er);
            double* D = G.ed + (int64_t)e * EG_ED;
#pragma unroll
            for (int r = 0; r < 7; r++) { S.err[le][r] = er[r]; D[ED_ERR + r] = er[r]; }
            D[ED_CHI] = eg_chi2(er);
        }
    }
    __syncthreads();
    // constructQuadraticForm: A'A, A'B, B'B and A'(-e), B'(-e), each a sum over the error's rows in index order
    for (int q = tid; q < EG_LIN_EDGES * 161; q += EG_LIN_T) {
        const int l2 = q / 161, w = q % 161, e2 = blockIdx.x * EG_LIN_EDGES + l2;
        if (e2 >= nE) break;
        double* D = G.ed + (int64_t)e2 * EG_ED;
        const double* Ji = S.J[l2][0];
        const double* Jj = S.J[l2][1];
        double s = 0.0;
        if (w < 147) {
            const int blk = w / 49, a = (w % 49) / 7, b = w % 7;
            const double* Pa = blk == 2 ? Jj : Ji;
            const double* Pb = blk == 0 ? Ji : Jj;
#pragma unroll
            for (int r = 0; r < 7; r++) s += Pa[r * 7 + a] * Pb[r * 7 + b];
            D[ED_HII + w] = s;
        } else {
            const int sd = (w - 147) / 7, a = (w - 147) % 7;
            const double* Pa = sd ? Jj : Ji;
#pragma unroll
            for (int r = 0; r < 7; r++) s += Pa[r * 7 + a] * (-S.err[l2][r]);
            D[ED_BI + (w - 147)] = s;
        }
    }
}

// One wave per block row: lane a*7 + b < 49 owns entry (a, b) of every block of the row, lanes 49..55 own b
__global__ __launch_bounds__(64) void k_eg_assemble(EgArgs G)
{
    if (G.st->stop) return;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= G.st->nFree || lane >= 56) return;
    const int v = G.rowKf[r], lo = G.first[r];
    double* Row = G.A + (int64_t)G.off[r] * 49;
    const int a = lane / 7, b = lane % 7;
    if (lane < 49)
        for (int k = 0; k <= r - lo; k++) Row[(int64_t)k * 49 + lane] = 0.0;
    double bs = 0.0;
    for (int k = G.incStart[v]; k < G.incStart[v + 1]; k++) {
        const int e = G.incEdge[k];
        const EgEdge& E = G.edges[e];
        const bool isI = E.v0 == v;
        const double* D = G.ed + (int64_t)e * EG_ED;
        if (lane >= 49) { bs += D[(isI ? ED_BI : ED_BJ) + (lane - 49)]; continue; }
        Row[(int64_t)(r - lo) * 49 + lane] += D[(isI ? ED_HII : ED_HJJ) + lane];
        const int u = G.sys[isI ? E.v1 : E.v0];
        if (u >= 0 && u < r) Row[(int64_t)(u - lo) * 49 + lane] += isI ? D[ED_HIJ + lane] : D[ED_HIJ + b * 7 + a];
    }
    if (lane >= 49) G.b[r * 7 + (lane - 49)] = bs;
}

struct EgStepShared { double part[EG_T / 64]; double panel[EG_PANEL][49]; double diag[49]; int ok; };

__device__ __forceinline__ double* eg_block(const EgArgs& G, double* M, int row, int col) { return M + ((int64_t)G.off[row] + (col - G.first[row])) * 49; }

// L L' of the damped skyline in G.L; false = a pivot is not positive
__device__ bool eg_factor(const EgArgs& G, EgStepShared& S, int n, double lambda)
{
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)G.off[n] * 49;
    for (int64_t k = tid; k < total; k += EG_T) G.L[k] = G.A[k];
    __syncthreads();
    for (int k = tid; k < n * 7; k += EG_T) {                                        // setLambda: the diagonal + lambda
        double* D = eg_block(G, G.L, k / 7, k / 7);
        D[(k % 7) * 8] += lambda;
    }
    if (tid == 0) S.ok = 1;
    __syncthreads();
    for (int kb = 0; kb < n; kb++) {
        double* D = eg_block(G, G.L, kb, kb);
        if (tid == 0) {
            double M[49];
            for (int k = 0; k < 49; k++) M[k] = D[k];
            bool ok = true;
            for (int j = 0; j < 7 && ok; j++) {
                if (!(M[j * 8] > 0.0)) { ok = false; break; }
                const double rk = __dsqrt_rn(M[j * 8]);
                M[j * 8] = rk;
                for (int i = j + 1; i < 7; i++) M[i * 7 + j] /= rk;
                for (int i = j + 1; i < 7; i++)
                    for (int c = j + 1; c <= i; c++) M[i * 7 + c] -= M[i * 7 + j] * M[c * 7 + j];
            }
            for (int k = 0; k < 49; k++) { D[k] = M[k]; S.diag[k] = M[k]; }
            if (!ok) S.ok = 0;
        }
        __syncthreads();
        if (!S.ok) return false;
        const int cs = G.colStart[kb], m = G.colStart[kb + 1] - cs;
        // the panel: row (ib, a) of column block kb, by columns
        for (int q = tid; q < m * 7; q += EG_T) {
            const int p = q / 7, a = q % 7;
            double* Bk = eg_block(G, G.L, G.colRows[cs + p], kb) + a * 7;
            double v[7];
            for (int c = 0; c < 7; c++) {
                double t = Bk[c];
                for (int k = 0; k < c; k++) t -= v[k] * S.diag[c * 7 + k];
                v[c] = t / S.diag[c * 8];
            }
            for (int c = 0; c < 7; c++) { Bk[c] = v[c]; if (p < EG_PANEL) S.panel[p][a * 7 + c] = v[c]; }
        }
        __syncthreads();
        // the trailing blocks (ib, jb), jb <= ib, of the rows that reach kb
        for (int q = tid; q < m * m * 49; q += EG_T) {
            const int pr = q / 49, w = q % 49, pa = pr / m, pb = pr % m;
            const int ib = G.colRows[cs + pa], jb = G.colRows[cs + pb];
            if (jb > ib) continue;
            const int a = w / 7, b = w % 7;
            const double* La = pa < EG_PANEL ? &S.panel[pa][a * 7] : eg_block(G, G.L, ib, kb) + a * 7;
            const double* Lb = pb < EG_PANEL ? &S.panel[pb][b * 7] : eg_block(G, G.L, jb, kb) + b * 7;
            double* T = eg_block(G, G.L, ib, jb) + w;
            double t = *T;
#pragma unroll
            for (int k = 0; k < 7; k++) t -= La[k] * Lb[k];
            *T = t;
        }
        __syncthreads();
    }
    return true;
}

// L y = b by columns, then L' x = y by columns from the last; G.x holds the result
__device__ void eg_solve(const EgArgs& G, EgStepShared& S, int n)
{
    const int tid = threadIdx.x;
    for (int k = tid; k < n * 7; k += EG_T) G.x[k] = G.b[k];
    __syncthreads();
    for (int kb = 0; kb < n; kb++) {
        const double* D = eg_block(G, G.L, kb, kb);
        double* y = G.x + kb * 7;
        if (tid == 0)
            for (int c = 0; c < 7; c++) {
                double t = y[c];
                for (int k = 0; k < c; k++) t -= D[c * 7 + k] * y[k];
                y[c] = t / D[c * 8];
            }
        __syncthreads();
        const int cs = G.colStart[kb], m = G.colStart[kb + 1] - cs;
        for (int q = tid; q < m * 7; q += EG_T) {
            const int ib = G.colRows[cs + q / 7], a = q % 7;
            const double* Bk = eg_block(G, G.L, ib, kb) + a * 7;
            double t = G.x[ib * 7 + a];
#pragma unroll
            for (int k = 0; k < 7; k++) t -= Bk[k] * y[k];
            G.x[ib * 7 + a] = t;
        }
        __syncthreads();
    }
    for (int kb = n - 1; kb >= 0; kb--) {
        const double* D = eg_block(G, G.L, kb, kb);
        double* x = G.x + kb * 7;
        if (tid == 0)
            for (int c = 6; c >= 0; c--) {
                double t = x[c];
                for (int k = 6; k > c; k--) t -= D[k * 7 + c] * x[k];
                x[c] = t / D[c * 8];
            }
        __syncthreads();
        const int lo = G.first[kb];
        for (int q = tid; q < (kb - lo) * 7; q += EG_T) {
            const int jb = lo + q / 7, b = q % 7;
            const double* Bk = eg_block(G, G.L, kb, jb);
            double t = G.x[jb * 7 + b];
#pragma unroll
            for (int k = 6; k >= 0; k--) t -= Bk[k * 7 + b] * x[k];
            G.x[jb * 7 + b] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(EG_T) void k_eg_step(EgArgs G)
{
    __shared__ EgStepShared S;
    EgState st = *G.st;
    if (st.stop) return;
    const int tid = threadIdx.x, n = st.nFree, nE = st.nEdges;
    // activeRobustChi2 at the estimates (k_eg_linearize left each edge's chi2)
    double acc = 0.0;
    for (int e = tid; e < nE; e += EG_T) acc += G.ed[(int64_t)e * EG_ED + ED_CHI];
    double currentChi = g2o_block_sum(S.part, acc);
    const double iniChi = currentChi;
    if (!g2o_finite(currentChi)) {
        if (tid == 0) { G.st->status = PGORB_EG_NONFINITE; G.st->stop = 1; }
        return;
    }
    G2oLm lm = st.lm;
    int trials = st.trials;
    if (st.iter == 0) g2o_lm_begin(lm, 1e-16);                                       // computeLambdaInit: _userLambdaInit > 0
    double rho = 0.0;
    int qmax = 0;
    do {
        const double lambda = lm.lambda;
        const bool ok2 = eg_factor(G, S, n, lambda);
        if (ok2) eg_solve(G, S, n);
        else {
            __syncthreads();
            for (int k = tid; k < n * 7; k += EG_T) G.x[k] = 0.0;                    // a failed factorisation: the trial stays at the estimates
        }
        __syncthreads();
        // update(): oplusImpl zeroes update[6] inside the solver's x under _fix_scale, so computeScale sees it
        for (int r = tid; r < n; r += EG_T) {
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; k++) u[k] = G.x[r * 7 + k];
            if (G.fixScale) { u[6] = 0.0; G.x[r * 7 + 6] = 0.0; }
            const int v = G.rowKf[r];
            G.trial[v] = os_mul(os_exp(u), G.est[v]);
        }
        __syncthreads();
        double sc = 0.0;
        for (int k = tid; k < n * 7; k += EG_T) sc += G.x[k] * (lambda * G.x[k] + G.b[k]);
        const double scale = g2o_block_sum(S.part, sc);
        acc = 0.0;
        for (int e = tid; e < nE; e += EG_T) {
            const EgEdge& E = G.edges[e];
            double er[7];
            eg_error(E.C, G.trial[E.v0], G.trial[E.v1], er);
            acc += eg_chi2(er);
        }
        const double tempChi = g2o_block_sum(S.part, acc);
        if (g2o_lm_decide(lm, currentChi, tempChi, ok2, scale, rho)) {
            for (int r = tid; r < n; r += EG_T) { const int v = G.rowKf[r]; G.est[v] = G.trial[v]; }      // discardTop
        } else {
            for (int r = tid; r < n; r += EG_T) { const int v = G.rowKf[r]; G.trial[v] = G.est[v]; }      // pop
        }
        __syncthreads();
        qmax++; trials++;
    } while (g2o_lm_again(rho, qmax));
    const bool stop = g2o_lm_stop(lm, iniChi, currentChi, qmax, rho);
    if (tid == 0) {
        EgState* P = G.st;
        P->lm = lm; P->trials = trials; P->its = st.its + 1; P->iter = st.iter + 1;
        P->stop = (stop || st.iter + 1 >= G.iterations) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_eg_finish(EgArgs G)
{
    const EgState st = *G.st;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keepIn = st.status != 0;                                              // outputs = inputs
    const OsSim* est = keepIn ? G.scw : G.est;
    if (g < G.nkf) {
        const int i = (int)g;
        pgorb_kf_pose o = G.pose[i];
        OsSim S;
        memset(&S, 0, sizeof(S));
        if (!eg_bad(G, i)) {
            S = est[i];
            if (!keepIn && G.deg[i] > 0) {
                // [R | t/s] (:1001-1007), Converter::toCvSE3 to float, SetPose's Ow = -Rcw.t()*tcw
                lp_pose_from_sim3(S, o);
            }
        }
        G.poseOut[i] = o;
        memcpy(&G.simOut[i], &S, sizeof(S));
    }
    if (G.edgeOut && g < st.nEdges) {
        const EgEdge& E = G.edges[g];
        double er[7];
        eg_error(E.C, est[E.v0], est[E.v1], er);
        pgorb_eg_edge o;
        o.i = E.v0; o.j = E.v1; o.kind = E.kind; o.pad = 0; o.chi2 = eg_chi2(er);
        G.edgeOut[g] = o;
    }
    if (!keepIn && g < G.npoints && !(G.pbad && G.pbad[g])) {                        // :1013-1040
        const int r = G.pref[g];
        if (eg_kf(G, r)) {
            float* pos = G.pts[g].pos;
            double x, y, z, X, Y, Z;
            lp_map(G.scw[r], (double)pos[0], (double)pos[1], (double)pos[2], x, y, z);
            lp_map(os_inverse(G.est[r]), x, y, z, X, Y, Z);
            pos[0] = __double2float_rn(X); pos[1] = __double2float_rn(Y); pos[2] = __double2float_rn(Z);
        }
    }
    if (g == 0 && G.info) {
        int32_t* I = G.info;
        I[0] = st.status; I[1] = st.nVert; I[2] = keepIn ? 0 : st.nFree; I[3] = st.nKind[0]; I[4] = st.nKind[1]; I[5] = st.nKind[2];
        I[6] = st.nKind[3]; I[7] = keepIn ? 0 : st.its; I[8] = keepIn ? 0 : st.trials; I[9] = st.env;
    }
}

extern "C" {

int pgorb_optimize_essential_graph_device(pgorb_ctx* c, int nkf, const uint64_t* d_kf_id, const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad,
        int loop_kf, int cur_kf, int fix_scale, const uint8_t* d_has_corrected, const pgorb_sim3d* d_corrected,
        const uint8_t* d_has_non_corrected, const pgorb_sim3d* d_non_corrected, int nloop_conn, const int32_t* d_loop_conn,
        const int32_t* d_parent, const int32_t* d_loop_edge_start, const int32_t* d_loop_edge, int nloop_edges,
        const int32_t* d_covis_start, const int32_t* d_covis, const int32_t* d_covis_weight, int ncovis, int min_feat, int iterations,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_point_ref_kf,
        pgorb_sim3d* d_sim3_out, pgorb_kf_pose* d_pose_out, pgorb_eg_edge* d_edge_out, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nkf < 0 || nloop_conn < 0 || nloop_edges < 0 || ncovis < 0 || npoints < 0 || iterations < 0 || !d_info ||
        (nkf && (!d_kf_id || !d_pose || !d_parent || !d_loop_edge_start || !d_covis_start || !d_sim3_out || !d_pose_out || d_pose_out == d_pose)) ||
        (d_has_corrected && !d_corrected) || (d_has_non_corrected && !d_non_corrected) || (nloop_conn && !d_loop_conn) ||
        (nloop_edges && !d_loop_edge) || (ncovis && (!d_covis || !d_covis_weight)) || (npoints && (!d_points || !d_point_ref_kf)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_optimize_essential_graph_device");
    if (nkf > PGORB_EG_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_essential_graph: more than PGORB_EG_MAX_KF key frames");
    const int64_t ncand64 = (int64_t)nloop_conn + nkf + nloop_edges + ncovis;
    if (ncand64 > PGORB_EG_MAX_EDGES) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_essential_graph: more than PGORB_EG_MAX_EDGES candidate edges");
    hipStream_t s = (hipStream_t)stream;
    EgArgs G;
    memset(&G, 0, sizeof(G));
    G.nkf = nkf; G.id = d_kf_id; G.pose = d_pose; G.bad = d_kf_bad; G.loopKf = loop_kf; G.curKf = cur_kf; G.fixScale = fix_scale ? 1 : 0;
    G.hasCor = d_has_corrected; G.cor = (const OsSim*)d_corrected; G.hasNon = d_has_non_corrected; G.non = (const OsSim*)d_non_corrected;
    G.nlc = nloop_conn; G.lc = d_loop_conn; G.parent = d_parent; G.leStart = d_loop_edge_start; G.le = d_loop_edge; G.nle = nloop_edges;
    G.cvStart = d_covis_start; G.cv = d_covis; G.cvW = d_covis_weight; G.ncv = ncovis; G.minFeat = min_feat; G.iterations = iterations;
    G.npoints = npoints; G.pts = d_points; G.pbad = d_point_bad; G.pref = d_point_ref_kf;
    G.simOut = d_sim3_out; G.poseOut = d_pose_out; G.edgeOut = d_edge_out; G.info = d_info;
    G.ncand = (int)ncand64;
    G.envCap = (int)std::min<int64_t>(PGORB_EG_MAX_ENVELOPE_BLOCKS, (int64_t)nkf * (nkf + 1) / 2);
    // the arena: 8-byte items first
    const size_t K = (size_t)std::max(nkf, 1), Cn = (size_t)std::max(G.ncand, 1), V = (size_t)std::max(G.envCap, 1);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t oSt = take(sizeof(EgState)), oEst = take(K * 64), oTrial = take(K * 64), oScw = take(K * 64), oEdges = take(Cn * sizeof(EgEdge)),
                 oEd = take(Cn * EG_ED * 8), oA = take(V * 49 * 8), oL = take(V * 49 * 8), oB = take(K * 7 * 8), oX = take(K * 7 * 8),
                 oSys = take(K * 4), oRowKf = take(K * 4), oDeg = take(K * 4), oIncStart = take((K + 1) * 4), oIncEdge = take(Cn * 8),
                 oCursor = take(K * 4), oKeep = take(Cn * 4), oRank = take(Cn * 4), oFirst = take(K * 4), oOff = take((K + 1) * 4),
                 oColStart = take((K + 1) * 4), oColRows = take(V * 4);
    void* scr;
    int rc = pg_ctx_scratch(c, at, s, &scr);
    if (rc) return rc;
    uint8_t* p = (uint8_t*)scr;
    G.st = (EgState*)(p + oSt); G.est = (OsSim*)(p + oEst); G.trial = (OsSim*)(p + oTrial); G.scw = (OsSim*)(p + oScw);
    G.edges = (EgEdge*)(p + oEdges); G.ed = (double*)(p + oEd); G.A = (double*)(p + oA); G.L = (double*)(p + oL);
    G.b = (double*)(p + oB); G.x = (double*)(p + oX); G.sys = (int32_t*)(p + oSys); G.rowKf = (int32_t*)(p + oRowKf);
    G.deg = (int32_t*)(p + oDeg); G.incStart = (int32_t*)(p + oIncStart); G.incEdge = (int32_t*)(p + oIncEdge);
    G.cursor = (int32_t*)(p + oCursor); G.keep = (int32_t*)(p + oKeep); G.rank = (int32_t*)(p + oRank); G.first = (int32_t*)(p + oFirst);
    G.off = (int32_t*)(p + oOff); G.colStart = (int32_t*)(p + oColStart); G.colRows = (int32_t*)(p + oColRows);
    const unsigned linBlocks = (unsigned)((G.ncand + EG_LIN_EDGES - 1) / EG_LIN_EDGES);
    hipLaunchKernelGGL(k_eg_prepare, dim3(1), dim3(EG_PREP_T), 0, s, G);
    for (int it = 0; it < iterations && G.ncand > 0 && nkf > 0; it++) {
        hipLaunchKernelGGL(k_eg_linearize, dim3(linBlocks), dim3(EG_LIN_T), 0, s, G);
        hipLaunchKernelGGL(k_eg_assemble, dim3((unsigned)nkf), dim3(64), 0, s, G);
        hipLaunchKernelGGL(k_eg_step, dim3(1), dim3(EG_T), 0, s, G);
    }
    const int64_t items = std::max<int64_t>(std::max<int64_t>(nkf, npoints), std::max<int64_t>(G.ncand, 1));
    hipLaunchKernelGGL(k_eg_finish, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, G);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "an essential-graph launch failed");
    return pg_ctx_scratch_done(c, s);
}

static bool eg_sim3_ok(const pgorb_sim3d& S)
{
    for (int k = 0; k < 4; k++) if (!std::isfinite(S.r[k])) return false;
    for (int k = 0; k < 3; k++) if (!std::isfinite(S.t[k])) return false;
    return std::isfinite(S.s) && S.s > 0.0;
}

int pgorb_optimize_essential_graph(pgorb_ctx* c, int nkf, const uint64_t* kf_id, const pgorb_kf_pose* pose, const uint8_t* kf_bad,
        int loop_kf, int cur_kf, int fix_scale, const uint8_t* has_corrected, const pgorb_sim3d* corrected,
        const uint8_t* has_non_corrected, const pgorb_sim3d* non_corrected, int nloop_conn, const int32_t* loop_conn,
        const int32_t* parent, const int32_t* loop_edge_start, const int32_t* loop_edge, const int32_t* covis_start, const int32_t* covis,
        const int32_t* covis_weight, int min_feat, int iterations, int npoints, pgorb_map_point* points, const uint8_t* point_bad,
        const int32_t* point_ref_kf, pgorb_sim3d* sim3_out, pgorb_kf_pose* pose_out, pgorb_eg_edge* edge_out, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* why = nullptr;
    int nle = 0, ncv = 0;
    if (nkf < 0 || nloop_conn < 0 || npoints < 0) why = "a count is negative";
    else if (iterations < 0) why = "iterations is negative";
    else if ((nkf && (!kf_id || !pose || !parent || !loop_edge_start || !covis_start || !sim3_out || !pose_out)) || (has_corrected && !corrected) ||
             (has_non_corrected && !non_corrected) || (nloop_conn && !loop_conn) || (npoints && (!points || !point_ref_kf)))
        why = "an array that is read or written is NULL";
    else if (nkf && (loop_kf < 0 || loop_kf >= nkf || cur_kf < 0 || cur_kf >= nkf)) why = "loop_kf or cur_kf is out of range";
    else if (!nkf && (nloop_conn || npoints)) why = "a list names a key frame of none";
    for (int i = 0; !why && i < nkf; i++) {
        if (i && !(kf_id[i] > kf_id[i - 1])) why = "kf_id is not strictly rising";
        else if (parent[i] < -1 || parent[i] >= nkf || parent[i] == i) why = "a parent is out of range";
        else if ((has_corrected && has_corrected[i] && !eg_sim3_ok(corrected[i])) || (has_non_corrected && has_non_corrected[i] && !eg_sim3_ok(non_corrected[i])))
            why = "a Sim3 is not finite or its scale is not positive";
        else for (int k = 0; k < 12; k++) if (!std::isfinite(pose[i].Tcw[k])) why = "a pose is not finite";
    }
    if (!why && nkf) {
        if (loop_edge_start[0] != 0 || covis_start[0] != 0) why = "a start array does not begin at 0";
        for (int i = 0; !why && i < nkf; i++)
            if (loop_edge_start[i + 1] < loop_edge_start[i] || covis_start[i + 1] < covis_start[i]) why = "a start array decreases";
        if (!why) {
            nle = loop_edge_start[nkf]; ncv = covis_start[nkf];
            if ((nle && !loop_edge) || (ncv && (!covis || !covis_weight))) why = "an array that is read or written is NULL";
        }
        for (int i = 0; !why && i < nkf; i++) {
            for (int k = loop_edge_start[i]; !why && k < loop_edge_start[i + 1]; k++)
                if (loop_edge[k] < 0 || loop_edge[k] >= nkf || loop_edge[k] == i) why = "a loop edge is out of range or names its own key frame";
            for (int k = covis_start[i]; !why && k < covis_start[i + 1]; k++)
                if (covis[k] < 0 || covis[k] >= nkf || covis[k] == i) why = "a covisible is out of range or names its own key frame";
        }
    }
    for (int k = 0; !why && k < nloop_conn; k++)
        if (loop_conn[k * 3] < 0 || loop_conn[k * 3] >= nkf || loop_conn[k * 3 + 1] < 0 || loop_conn[k * 3 + 1] >= nkf || loop_conn[k * 3] == loop_conn[k * 3 + 1])
            why = "a loop connection is out of range or joins a key frame to itself";
    for (int p = 0; !why && p < npoints; p++) {
        if (point_ref_kf[p] < -1 || point_ref_kf[p] >= nkf) why = "point_ref_kf is out of range";
        else if (!std::isfinite(points[p].pos[0]) || !std::isfinite(points[p].pos[1]) || !std::isfinite(points[p].pos[2])) why = "a point is not finite";
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_optimize_essential_graph: ") + why).c_str());
    if (nkf > PGORB_EG_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_essential_graph: more than PGORB_EG_MAX_KF key frames");
    const int64_t ncand = (int64_t)nloop_conn + nkf + nle + ncv;
    if (ncand > PGORB_EG_MAX_EDGES) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_essential_graph: more than PGORB_EG_MAX_EDGES candidate edges");
    if (!nkf) {
        if (info) { memset(info, 0, PGORB_EG_INFO * 4); info[0] = PGORB_EG_NOTHING; }
        return 0;
    }
    const size_t K = (size_t)nkf, NP = (size_t)std::max(npoints, 1), NC = (size_t)std::max<int64_t>(ncand, 1);
    PgHostCall s(c);
    const size_t oId = s.region(PG_UP, K * 8), oPose = s.region(PG_UP, K * sizeof(pgorb_kf_pose)), oBad = s.region(PG_UP, kf_bad ? K : 0),
                 oHc = s.region(PG_UP, has_corrected ? K : 0), oCor = s.region(PG_UP, has_corrected ? K * 64 : 0),
                 oHn = s.region(PG_UP, has_non_corrected ? K : 0), oNon = s.region(PG_UP, has_non_corrected ? K * 64 : 0),
                 oLc = s.region(PG_UP, (size_t)std::max(nloop_conn, 1) * 12), oPar = s.region(PG_UP, K * 4), oLs = s.region(PG_UP, (K + 1) * 4),
                 oLe = s.region(PG_UP, (size_t)std::max(nle, 1) * 4), oCs = s.region(PG_UP, (K + 1) * 4), oCv = s.region(PG_UP, (size_t)std::max(ncv, 1) * 4),
                 oCw = s.region(PG_UP, (size_t)std::max(ncv, 1) * 4), oPb = s.region(PG_UP, point_bad ? NP : 0), oRef = s.region(PG_UP, NP * 4),
                 oPts = s.region(PG_INOUT, NP * sizeof(pgorb_map_point)),
                 oSim = s.region(PG_DOWN, K * 64), oPo = s.region(PG_DOWN, K * sizeof(pgorb_kf_pose)), oEo = s.region(PG_DOWN, NC * sizeof(pgorb_eg_edge)),
                 oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oId, kf_id, K * 8); s.put(oPose, pose, K * sizeof(pgorb_kf_pose));
    if (kf_bad) s.put(oBad, kf_bad, K);
    if (has_corrected) { s.put(oHc, has_corrected, K); s.put(oCor, corrected, K * 64); }
    if (has_non_corrected) { s.put(oHn, has_non_corrected, K); s.put(oNon, non_corrected, K * 64); }
    s.put(oLc, loop_conn, (size_t)nloop_conn * 12, 0, (size_t)std::max(nloop_conn, 1) * 12);
    s.put(oPar, parent, K * 4); s.put(oLs, loop_edge_start, (K + 1) * 4); s.put(oCs, covis_start, (K + 1) * 4);
    s.put(oLe, loop_edge, (size_t)nle * 4, 0, (size_t)std::max(nle, 1) * 4);
    s.put(oCv, covis, (size_t)ncv * 4, 0, (size_t)std::max(ncv, 1) * 4);
    s.put(oCw, covis_weight, (size_t)ncv * 4, 0, (size_t)std::max(ncv, 1) * 4);
    if (point_bad) s.put(oPb, point_bad, (size_t)npoints, 0, NP);
    s.put(oRef, point_ref_kf, (size_t)npoints * 4, 0, NP * 4);
    s.put(oPts, points, (size_t)npoints * sizeof(pgorb_map_point), 0, NP * sizeof(pgorb_map_point));
    if ((rc = s.run([&] {
            return pgorb_optimize_essential_graph_device(c, nkf, s.dev<uint64_t>(oId), s.dev<pgorb_kf_pose>(oPose), kf_bad ? s.dev(oBad) : nullptr,
                loop_kf, cur_kf, fix_scale, has_corrected ? s.dev(oHc) : nullptr, s.dev<pgorb_sim3d>(oCor), has_non_corrected ? s.dev(oHn) : nullptr,
                s.dev<pgorb_sim3d>(oNon), nloop_conn, s.dev<int32_t>(oLc), s.dev<int32_t>(oPar), s.dev<int32_t>(oLs), s.dev<int32_t>(oLe), nle,
                s.dev<int32_t>(oCs), s.dev<int32_t>(oCv), s.dev<int32_t>(oCw), ncv, min_feat, iterations, npoints, s.dev<pgorb_map_point>(oPts),
                point_bad ? s.dev(oPb) : nullptr, s.dev<int32_t>(oRef), s.dev<pgorb_sim3d>(oSim), s.dev<pgorb_kf_pose>(oPo),
                s.dev<pgorb_eg_edge>(oEo), s.dev<int32_t>(oInfo), nullptr); }))) return rc;
    const int32_t* I = s.host<int32_t>(oInfo);
    if (info) memcpy(info, I, PGORB_EG_INFO * 4);
    memcpy(sim3_out, s.host(oSim), K * 64);
    memcpy(pose_out, s.host(oPo), K * sizeof(pgorb_kf_pose));
    const int nE = I[3] + I[4] + I[5] + I[6];
    if (edge_out && nE > 0) memcpy(edge_out, s.host(oEo), (size_t)nE * sizeof(pgorb_eg_edge));
    if (npoints) memcpy(points, s.host(oPts), (size_t)npoints * sizeof(pgorb_map_point));
    if (I[0] & PGORB_EG_LIMIT) return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_optimize_essential_graph: the envelope exceeds PGORB_EG_MAX_ENVELOPE_BLOCKS");
    return I[2];
}

}  // extern "C"
