// loop.hip -- loop closing's four matchers on gfx950, monocular: SearchByBoW(KF, KF), SearchBySim3, and the two that take Scw.
//
// Restates (thirdparty/orb-slam2):
//   ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)   src/ORBmatcher.cc:292-405
//   ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)            src/ORBmatcher.cc:981-1104
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)        src/ORBmatcher.cc:1106-1330
//   ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)                  src/ORBmatcher.cc:524-657
//   KeyFrame::GetFeaturesInArea / IsInImage / GetMapPoints                     src/KeyFrame.cc:672-716, 338-351
//
// The Scw forms both project a list of map points through the decomposed Scw (the caller's pgorb_kf_pose), apply the image, depth and
// viewing-angle tests, PredictScale, and scan the key frame's search window in the reference's (ix, iy, insertion) order for the
// first smallest descriptor distance among octaves [level - 1, level].  There is no chi-square test.  spAlreadyFound is the state
// on entry (:308, :997) and is never updated: a per-problem byte mask over the map-point table (k_loop_mark).
//   Fuse:  matching never reads the slots, so one lane per query matches from the entry state (k_fs3_match) and leaves an
//          atomicMin of its query index on the slot it matched; k_fs3_resolve then reads each slot's winner: it alone found the
//          slot empty (ADDED), every later query of the slot sees that query's point as the occupant (REPLACE_REQUESTED).
//   SearchByProjection:  an accepted query occupies its keypoint for every later query.  A query takes its smallest-distance
//          untaken candidate only if that distance is <= TH_LOW, so candidates above TH_LOW never change a decision and are
//          dropped: k_ps3_lists stores every query's remaining candidates in scan order (one lane per query), and
//          k_ps3_decide, one workgroup per problem, decides the queries in rounds of provably independent ones (see there).
//   SearchBySim3:  nothing depends on order.  One lane per (pair, direction, slot) projects the slot's point through its own key
//          frame's pose and the Sim3 into the other key frame -- BOTH directions with pKF1's camera (:1109-1112) -- and takes the
//          first smallest distance <= TH_HIGH (k_s3_match); one pass keeps the pairs that agree (k_s3_agree).
//   SearchByBoW(KF, KF):  a KF2 feature belongs to one vocabulary node, so vbMatched2 never crosses a node: one wave per (pair,
//          common node) walks KF1's features of the node in FeatureVector order, KF2's features of it one per lane
//          (k_bow_keyframes); one finishing wave per pair counts and applies the rotation histogram (k_bow_keyframes_finish).
// Every float operation follows the reference's cv::Mat arithmetic under the readings of DESIGN.md section 4.
#include "match_common.h"

#define LOOP_T 1024
#define LOOP_K 64                           // candidates a query's list holds; more: the query is evaluated in place
#define LOOP_OVER 0xFFFF
#define LOOP_NONE 0x7FFFFFFF

struct PgLoopBatch {
    const pgorb_keypoint* K; const uint8_t* D; const int32_t* n; int cap;
    const int32_t* gstart; const int32_t* gidx; const int32_t* kf; const pgorb_kf_pose* pose;
    const int32_t* slots;                  // Fuse: kf_point [nframes][cap]; SearchByProjection: matched_in [nprob][cap]; or null
    int slotsPerProblem;                   // 1: slots rows go by problem, 0: by key frame
    int npoints; const pgorb_map_point* pts; const uint8_t* pdesc; const uint8_t* pbad;
    int qcap; const int32_t* nq; const int32_t* queries;
    float minX, minY, maxX, maxY;          // the key frame's int bounds (KeyFrame.h:195-198) as float
    float invW, invH;                      // mfGridElementWidthInv / HeightInv of the Frame's float bounds
    float sf[PG_MAXL + 1]; int nlevels; float logSf; float th;
    uint8_t* found;                        // [nprob][npoints] spAlreadyFound
};

__device__ __forceinline__ int64_t loop_slot_row(const PgLoopBatch& B, int p, int f) { return (int64_t)(B.slotsPerProblem ? p : f) * B.cap; }
// the occupant of slot s on entry: a table index, or -1 (out of range counts as NULL)
__device__ __forceinline__ int loop_occupant(const PgLoopBatch& B, int64_t row, int s)
{
    if (!B.slots) return -1;
    const int o = B.slots[row + s];
    return (o >= 0 && o < B.npoints) ? o : -1;
}

// spAlreadyFound of every problem (the mask is zeroed before)
__global__ __launch_bounds__(256) void k_loop_mark(PgLoopBatch B)
{
    const int p = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, f = B.kf[p];
    const int n = min(max(B.n[f], 0), B.cap);
    if (s >= n) return;
    const int o = loop_occupant(B, loop_slot_row(B, p, f), s);
    if (o >= 0) B.found[(int64_t)p * B.npoints + o] = 1;
}

struct LoopQuery { float u, v, r; int lvl, cx0, cx1, cy0, cy1; };
// :316-367 / :1006-1058 for query point mp of problem p: false = the reference `continue`s before the descriptor loop
__device__ __forceinline__ bool loop_query(const PgLoopBatch& B, int p, int f, int mp, LoopQuery& Q)
{
    if (mp < 0 || mp >= B.npoints || (B.pbad && B.pbad[mp]) || B.found[(int64_t)p * B.npoints + mp]) return false;
    const pgorb_map_point P = B.pts[mp];
    const pgorb_kf_pose& C = B.pose[f];
    const float* T = C.Tcw;
    // p3Dc = Rcw*p3Dw + tcw: gemm's small-matrix path with tcw as C
    const float zc = cnm_f(__dadd_rn((double)cnm_dot3f(T[8], T[9], T[10], P.pos[0], P.pos[1], P.pos[2]), (double)T[11]));
    if (zc < 0.0f) return false;
    const float xc = cnm_f(__dadd_rn((double)cnm_dot3f(T[0], T[1], T[2], P.pos[0], P.pos[1], P.pos[2]), (double)T[3]));
    const float yc = cnm_f(__dadd_rn((double)cnm_dot3f(T[4], T[5], T[6], P.pos[0], P.pos[1], P.pos[2]), (double)T[7]));
    const float invz = __fdiv_rn(1.0f, zc);
    Q.u = __fadd_rn(__fmul_rn(C.fx, __fmul_rn(xc, invz)), C.cx);
    Q.v = __fadd_rn(__fmul_rn(C.fy, __fmul_rn(yc, invz)), C.cy);
    if (!(Q.u >= B.minX && Q.u < B.maxX && Q.v >= B.minY && Q.v < B.maxY)) return false;     // IsInImage (KeyFrame.cc:713-716)
    const float po0 = __fsub_rn(P.pos[0], C.Ow[0]), po1 = __fsub_rn(P.pos[1], C.Ow[1]), po2 = __fsub_rn(P.pos[2], C.Ow[2]);
    const float dist3D = cnm_f(cnm_normd(po0, po1, po2));                                 // cv::norm(PO)
    if (dist3D < __fmul_rn(0.8f, P.min_distance) || dist3D > __fmul_rn(1.2f, P.max_distance)) return false;
    // PO.dot(Pn) < 0.5*dist, in double
    if (cnm_dotd(po0, po1, po2, P.normal[0], P.normal[1], P.normal[2]) < __dmul_rn(0.5, (double)dist3D)) return false;
    Q.lvl = pg_predict_scale(P.max_distance, dist3D, B.logSf, B.nlevels);
    Q.r = __fmul_rn(B.th, B.sf[Q.lvl]);
    return sfi_window(Q.u, Q.v, Q.r, B.minX, B.minY, B.invW, B.invH, Q.cx0, Q.cx1, Q.cy0, Q.cy1);
}

// the window of Q over key frame f in the reference's order: visit(idx, distance) for every keypoint inside the radius whose
// octave lies in [level - 1, level] and that skip(idx) does not exclude; returns whether vIndices was non-empty
template <class Skip, class Visit>
__device__ __forceinline__ bool loop_scan(const PgLoopBatch& B, int f, int mp, const LoopQuery& Q, Skip&& skip, Visit&& visit)
{
    const int cap = B.cap;
    const pgorb_keypoint* __restrict__ K = B.K + (int64_t)f * cap;
    const uint8_t* __restrict__ D = B.D + (int64_t)f * cap * 32;
    const int32_t* __restrict__ gstart = B.gstart + (int64_t)f * (PGORB_GRID_CELLS + 1);
    const int32_t* __restrict__ gidx = B.gidx + (int64_t)f * cap;
    const uint4 q0 = reinterpret_cast<const uint4*>(B.pdesc + (int64_t)mp * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.pdesc + (int64_t)mp * 32)[1];
    bool any = false;
    for (int ix = Q.cx0; ix <= Q.cx1; ix++)                                               // KeyFrame::GetFeaturesInArea
        for (int iy = Q.cy0; iy <= Q.cy1; iy++) {
            const int c = ix * PGORB_GRID_ROWS + iy;
            for (int j = gstart[c], je = gstart[c + 1]; j < je; j++) {
                const int idx = gidx[j];
                if (idx < 0 || idx >= cap) continue;
                const pgorb_keypoint kp = K[idx];
                if (!(fabsf(__fsub_rn(kp.x, Q.u)) < Q.r && fabsf(__fsub_rn(kp.y, Q.v)) < Q.r)) continue;
                any = true;
                if (skip(idx)) continue;
                const int o = kp.octave;
                if (o < Q.lvl - 1 || o > Q.lvl || o < 0) continue;
                visit(idx, sfi_distance(q0, q1, D + (int64_t)idx * 32));
            }
        }
    return any;
}

// ---- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) ----
__global__ __launch_bounds__(256) void k_fs3_match(PgLoopBatch B, int32_t* __restrict__ best, int32_t* __restrict__ dist,
                                                   int32_t* __restrict__ act, int32_t* __restrict__ head)
{
    const int p = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const int nq = min(max(B.nq[p], 0), B.qcap);
    if (q >= nq) return;
    const int64_t qi = (int64_t)p * B.qcap + q;
    const int f = B.kf[p], mp = B.queries[qi];
    int a = PGORB_FUSE_SKIPPED, bi = -1, bd = -1;
    LoopQuery Q;
    if (loop_query(B, p, f, mp, Q)) {
        int d1 = 256, i1 = -1;
        const bool any = loop_scan(B, f, mp, Q, [](int) { return false; },
                                   [&](int idx, int d) { if (d < d1) { d1 = d; i1 = idx; } });      // :1078-1082
        if (any) {
            bi = i1; bd = d1;
            a = PGORB_FUSE_NO_MATCH;
            if (d1 <= TH_LOW) { a = PGORB_FUSE_ADDED; atomicMin(&head[(int64_t)p * B.cap + i1], q); }   // provisional: k_fs3_resolve
        }
    }
    best[qi] = bi; dist[qi] = bd; act[qi] = a;
}

__global__ __launch_bounds__(256) void k_fs3_resolve(PgLoopBatch B, const int32_t* __restrict__ best, const int32_t* __restrict__ dist,
                                                     const int32_t* __restrict__ act, const int32_t* __restrict__ head,
                                                     int32_t* __restrict__ actOut, int32_t* __restrict__ replaceOut,
                                                     int32_t* __restrict__ bestOut, int32_t* __restrict__ distOut,
                                                     int32_t* __restrict__ slotsOut, int32_t* __restrict__ nfused)
{
    const int p = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, f = B.kf[p];
    const int nq = min(max(B.nq[p], 0), B.qcap), n = min(max(B.n[f], 0), B.cap);
    const int64_t rowQ = (int64_t)p * B.qcap, rowS = (int64_t)p * B.cap, rowIn = loop_slot_row(B, p, f);
    if (slotsOut && t < n) {
        const int o = loop_occupant(B, rowIn, t), h = head[rowS + t];
        slotsOut[rowS + t] = o >= 0 ? o : (h < nq ? B.queries[rowQ + h] : -1);
    }
    bool fused = false;
    if (t < nq) {
        int a = act[rowQ + t], rep = -1;
        const int s = best[rowQ + t];
        if (a == PGORB_FUSE_ADDED) {
            fused = true;
            const int o = loop_occupant(B, rowIn, s);
            if (o >= 0) {                                                              // :1089-1093
                if (B.pbad && B.pbad[o]) a = PGORB_FUSE_KF_POINT_BAD;
                else { a = PGORB_FUSE_REPLACE_REQUESTED; rep = o; }
            } else {
                const int w = head[rowS + s];                                          // the first matched query of the slot added its point
                if (w != t) { a = PGORB_FUSE_REPLACE_REQUESTED; rep = B.queries[rowQ + w]; }
            }
        }
        actOut[rowQ + t] = a;
        replaceOut[rowQ + t] = rep;
        if (bestOut) bestOut[rowQ + t] = s;
        if (distOut) distOut[rowQ + t] = dist[rowQ + t];
    }
    const unsigned long long m = __ballot(fused);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nfused[p], __popcll(m));
}

// ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) ----
// list entry: distance << 24 | list position << 16 | keypoint index: the smallest untaken entry is the reference's choice
__global__ __launch_bounds__(256) void k_ps3_lists(PgLoopBatch B, uint32_t* __restrict__ lists, uint16_t* __restrict__ cnt)
{
    const int p = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const int nq = min(max(B.nq[p], 0), B.qcap);
    if (q >= nq) return;
    const int64_t qi = (int64_t)p * B.qcap + q;
    const int f = B.kf[p], mp = B.queries[qi];
    const int64_t rowIn = loop_slot_row(B, p, f);
    int c = 0;
    LoopQuery Q;
    if (loop_query(B, p, f, mp, Q)) {
        uint32_t* L = lists + qi * LOOP_K;
        loop_scan(B, f, mp, Q, [&](int idx) { return loop_occupant(B, rowIn, idx) >= 0; },           // :377 on the entry state
                  [&](int idx, int d) {
                      if (d > TH_LOW) return;
                      if (c < LOOP_K) L[c] = ((uint32_t)d << 24) | ((uint32_t)c << 16) | (uint32_t)idx;
                      c++;
                  });
    }
    cnt[qi] = (uint16_t)(c > LOOP_K ? LOOP_OVER : c);
}

// One workgroup per problem.  What query q decides depends on earlier queries only through the taken state of the keypoints in its
// own list, and a query only ever takes a keypoint of its list.  Round: minq[i] = the smallest undecided query that lists the
// untaken keypoint i; q is ready when minq[i] == q for every untaken i of its list, i.e. no undecided earlier query can take any
// of them: its view is final and it takes its smallest entry (two ready queries never list the same untaken keypoint: the later
// one would not be ready).  The smallest undecided query is always ready, so the rounds end.  A query whose list overflowed waits
// until it is the smallest undecided one, holds back everything behind it, and is evaluated in place.
__global__ __launch_bounds__(LOOP_T) void k_ps3_decide(PgLoopBatch B, const uint32_t* __restrict__ lists, const uint16_t* __restrict__ cnt,
                                                       int32_t* __restrict__ pendA, int32_t* __restrict__ pendB, int32_t* __restrict__ dec,
                                                       int32_t* __restrict__ assignedOut, int32_t* __restrict__ matchedOut,
                                                       int32_t* __restrict__ nmatches)
{
    const int p = blockIdx.x, tid = threadIdx.x, f = B.kf[p], cap = B.cap;
    const int n = min(max(B.n[f], 0), cap), nq = min(max(B.nq[p], 0), B.qcap);
    const int64_t rowQ = (int64_t)p * B.qcap, rowS = (int64_t)p * cap, rowIn = loop_slot_row(B, p, f);
    uint32_t* minq = reinterpret_cast<uint32_t*>(pg_sfi_smem);                      // [cap]
    uint8_t* taken = reinterpret_cast<uint8_t*>(minq + cap);                        // [cap]
    __shared__ int sNext, sCount, sMinOver, sMinAll;
    if (tid == 0) { sNext = 0; sCount = 0; }
    for (int s = tid; s < cap; s += LOOP_T) {
        const int o = s < n ? loop_occupant(B, rowIn, s) : -1;
        taken[s] = o >= 0;
        if (s < n) { assignedOut[rowS + s] = -1; if (matchedOut) matchedOut[rowS + s] = o; }
    }
    __syncthreads();
    for (int q = tid; q < nq; q += LOOP_T)
        if (cnt[rowQ + q]) pendA[rowQ + atomicAdd(&sNext, 1)] = q;
    __syncthreads();
    int npend = sNext;
    int32_t* pend = pendA + rowQ;
    int32_t* next = pendB + rowQ;
    int count = 0;
    while (npend > 0) {
        __syncthreads();
        for (int k = tid; k < cap; k += LOOP_T) minq[k] = 0xFFFFFFFFu;
        if (tid == 0) { sNext = 0; sMinOver = LOOP_NONE; sMinAll = LOOP_NONE; }
        __syncthreads();
        for (int i = tid; i < npend; i += LOOP_T) {
            const int q = pend[i], c = cnt[rowQ + q];
            atomicMin(&sMinAll, q);
            if (c == LOOP_OVER) { atomicMin(&sMinOver, q); continue; }
            for (int k = 0; k < c; k++) {
                const int idx = (int)(lists[(rowQ + q) * LOOP_K + k] & 0xFFFFu);
                if (!taken[idx]) atomicMin(&minq[idx], (uint32_t)q);
            }
        }
        __syncthreads();
        const int minOver = sMinOver, minAll = sMinAll;
        // ready queries decide from the state as it is (reads only): dec = the keypoint, -1 none, -2 not ready
        for (int i = tid; i < npend; i += LOOP_T) {
            const int q = pend[i], c = cnt[rowQ + q];
            int d = -2;
            if (c == LOOP_OVER) {
                if (q == minAll) {
                    const int mp = B.queries[rowQ + q];
                    LoopQuery Q;
                    int d1 = 256, i1 = -1;
                    if (loop_query(B, p, f, mp, Q))
                        loop_scan(B, f, mp, Q, [&](int idx) { return taken[idx] != 0; },
                                  [&](int idx, int dd) { if (dd < d1) { d1 = dd; i1 = idx; } });
                    d = d1 <= TH_LOW ? i1 : -1;
                }
            } else if (q < minOver) {
                uint32_t bestE = 0xFFFFFFFFu;
                bool ready = true;
                for (int k = 0; k < c; k++) {
                    const uint32_t e = lists[(rowQ + q) * LOOP_K + k];
                    const int idx = (int)(e & 0xFFFFu);
                    if (taken[idx]) continue;
                    if (minq[idx] != (uint32_t)q) { ready = false; break; }
                    bestE = min(bestE, e);
                }
                if (ready) d = bestE == 0xFFFFFFFFu ? -1 : (int)(bestE & 0xFFFFu);
            }
            dec[rowQ + q] = d;
        }
        __syncthreads();
        for (int i = tid; i < npend; i += LOOP_T) {
            const int q = pend[i], d = dec[rowQ + q];
            if (d == -2) { next[atomicAdd(&sNext, 1)] = q; continue; }
            if (d < 0) continue;
            taken[d] = 1;                                                            // :398-399
            assignedOut[rowS + d] = q;
            if (matchedOut) matchedOut[rowS + d] = B.queries[rowQ + q];
            count++;
        }
        __syncthreads();
        npend = sNext;
        int32_t* t = pend; pend = next; next = t;
    }
    atomicAdd(&sCount, count);
    __syncthreads();
    if (tid == 0) nmatches[p] = sCount;
}


// ---- SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) ----
struct PgSim3Batch { const int32_t* kf1; const int32_t* kf2; const pgorb_sim3* sim3; const uint8_t* already1; const uint8_t* already2; };

// blockIdx.z = direction: 0 projects KF1's points into KF2 (:1152-1229), 1 KF2's into KF1 (:1232-1309)
__global__ __launch_bounds__(256) void k_s3_match(PgLoopBatch B, PgSim3Batch E, int32_t* __restrict__ m1, int32_t* __restrict__ m2)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, dir = blockIdx.z;
    const int f1 = E.kf1[p], f2 = E.kf2[p];
    const int fs = dir ? f2 : f1, ft = dir ? f1 : f2;                                    // source and target key frame
    const int ns = min(max(B.n[fs], 0), B.cap);
    if (i >= ns) return;
    int32_t* out = (dir ? m2 : m1) + (int64_t)p * B.cap;
    const uint8_t* already = dir ? E.already2 : E.already1;
    int res = -1;
    const int mp = loop_occupant(B, (int64_t)fs * B.cap, i);
    if (mp >= 0 && !(already && already[(int64_t)p * B.cap + i]) && !(B.pbad && B.pbad[mp])) {
        const pgorb_map_point P = B.pts[mp];
        const float* T = B.pose[fs].Tcw;
        const pgorb_kf_pose& C1 = B.pose[f1];                                            // pKF1's fx, fy, cx, cy in both directions
        const pgorb_sim3& S = E.sim3[p];
        const float* M = dir ? S.sR12 : S.sR21;
        const float* t = dir ? S.t12 : S.t21;
        // p3Dc = Rw*p3Dw + tw, then sR*p3Dc + t: gemm's small-matrix path twice, the translation as C
        float a[3], b[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
            a[r] = cnm_f(__dadd_rn((double)cnm_dot3f(T[4 * r], T[4 * r + 1], T[4 * r + 2], P.pos[0], P.pos[1], P.pos[2]), (double)T[4 * r + 3]));
#pragma unroll
        for (int r = 0; r < 3; r++)
            b[r] = cnm_f(__dadd_rn((double)cnm_dot3f(M[3 * r], M[3 * r + 1], M[3 * r + 2], a[0], a[1], a[2]), (double)t[r]));
        LoopQuery Q;
        bool ok = !(b[2] < 0.0f);
        if (ok) {
            const float invz = __fdiv_rn(1.0f, b[2]);                                    // (float)(1.0/z): the double quotient rounds the same
            Q.u = __fadd_rn(__fmul_rn(C1.fx, __fmul_rn(b[0], invz)), C1.cx);
            Q.v = __fadd_rn(__fmul_rn(C1.fy, __fmul_rn(b[1], invz)), C1.cy);
            ok = Q.u >= B.minX && Q.u < B.maxX && Q.v >= B.minY && Q.v < B.maxY;
        }
        if (ok) {
            const float dist3D = cnm_f(cnm_normd(b[0], b[1], b[2]));                     // cv::norm of the camera-frame vector
            ok = !(dist3D < __fmul_rn(0.8f, P.min_distance) || dist3D > __fmul_rn(1.2f, P.max_distance));
            if (ok) {
                Q.lvl = pg_predict_scale(P.max_distance, dist3D, B.logSf, B.nlevels);
                Q.r = __fmul_rn(B.th, B.sf[Q.lvl]);
                ok = sfi_window(Q.u, Q.v, Q.r, B.minX, B.minY, B.invW, B.invH, Q.cx0, Q.cx1, Q.cy0, Q.cy1);
            }
        }
        if (ok) {
            int d1 = 0x7FFFFFFF, i1 = -1;
            loop_scan(B, ft, mp, Q, [](int) { return false; }, [&](int idx, int d) { if (d < d1) { d1 = d; i1 = idx; } });
            if (d1 <= TH_HIGH) res = i1;
        }
    }
    out[i] = res;
}

__global__ __launch_bounds__(256) void k_s3_agree(PgLoopBatch B, PgSim3Batch E, const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                  int32_t* __restrict__ match12, int32_t* __restrict__ nfound)
{
    const int p = blockIdx.y, i1 = blockIdx.x * 256 + threadIdx.x;
    const int n1 = min(max(B.n[E.kf1[p]], 0), B.cap), n2 = min(max(B.n[E.kf2[p]], 0), B.cap);
    bool ok = false;
    if (i1 < n1) {
        const int idx2 = m1[(int64_t)p * B.cap + i1];
        ok = idx2 >= 0 && idx2 < n2 && m2[(int64_t)p * B.cap + idx2] == i1;            // :1314-1327
        match12[(int64_t)p * B.cap + i1] = ok ? idx2 : -1;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nfound[p], __popcll(m));
}

// ---- SearchByBoW(pKF1, pKF2, vpMatches12) ----
// Differences from SearchByBoW(KeyFrame*, Frame&) (node_match.hip): bestDist1 < TH_LOW is strict (:600); KF2's side is masked by
// validity AND vbMatched2 (:578-582), and vbMatched2 is written only by an accepted match (:605); the output goes by KF1's feature.
struct PgKfBowBatch { PgFvBatch fv; const int32_t* kf1; const int32_t* kf2; const uint8_t* valid1; const uint8_t* valid2; };
#define KFBOW_WAVES 64           // waves per pair, each takes KF1's nodes a = wave, wave + 64, ...

__global__ __launch_bounds__(64) void k_bow_keyframes(PgKfBowBatch B, float nnratio, int checkOrientation, int32_t* __restrict__ m12,
                                                      int8_t* __restrict__ bins, uint8_t* matched2)
{
    const int p = blockIdx.y, cap = B.fv.cap, lane = threadIdx.x;
    const int f1 = B.kf1[p], f2 = B.kf2[p];
    const int n1 = min(max(B.fv.n[f1], 0), cap), n2 = min(max(B.fv.n[f2], 0), cap);
    const int nfv1 = min(max(B.fv.nfv[f1], 0), cap), nfv2 = min(max(B.fv.nfv[f2], 0), cap);
    const uint32_t* __restrict__ node1 = B.fv.fvNode + (int64_t)f1 * cap;
    const uint32_t* __restrict__ node2 = B.fv.fvNode + (int64_t)f2 * cap;
    const int32_t* __restrict__ start1 = B.fv.fvStart + (int64_t)f1 * (cap + 1);
    const int32_t* __restrict__ start2 = B.fv.fvStart + (int64_t)f2 * (cap + 1);
    const uint32_t* __restrict__ feat1 = B.fv.fvFeat + (int64_t)f1 * cap;
    const uint32_t* __restrict__ feat2 = B.fv.fvFeat + (int64_t)f2 * cap;
    const uint8_t* __restrict__ D1 = B.fv.D + (int64_t)f1 * cap * 32;
    const uint8_t* __restrict__ D2 = B.fv.D + (int64_t)f2 * cap * 32;
    const int64_t row = (int64_t)p * cap;
    for (int a = blockIdx.x; a < nfv1; a += KFBOW_WAVES) {
        const uint32_t id = node1[a];
        int lo = 0, hi = nfv2;                                                // KF2's entry of the same node (the ids ascend)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (node2[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo >= nfv2 || node2[lo] != id) continue;
        const int a0 = max(start1[a], 0), a1 = min(start1[a + 1], cap), b0 = max(start2[lo], 0), b1 = min(start2[lo + 1], cap);
        for (int ia = a0; ia < a1; ia++) {                                    // KF1's features of the node, in order (:556)
            const int idx1 = (int)feat1[ia];
            if ((unsigned)idx1 >= (unsigned)n1 || !B.valid1[row + idx1]) continue;     // !pMP1 || pMP1->isBad() (:560-564)
            const uint4 q0 = reinterpret_cast<const uint4*>(D1 + (int64_t)idx1 * 32)[0];
            const uint4 q1 = reinterpret_cast<const uint4*>(D1 + (int64_t)idx1 * 32)[1];
            unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;                      // the lane's two smallest (distance << 16 | list position)
            for (int k = lane; b0 + k < b1; k += 64) {
                const int idx2 = (int)feat2[b0 + k];
                if ((unsigned)idx2 >= (unsigned)n2) continue;
                if (matched2[row + idx2] || !B.valid2[row + idx2]) continue;  // vbMatched2[idx2] || !pMP2 || pMP2->isBad() (:578-582)
                const unsigned key = ((unsigned)sfi_distance(q0, q1, D2 + (int64_t)idx2 * 32) << 16) | (unsigned)k;
                if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
            }
            const unsigned w1 = wave_min_u32(k1);
            if (w1 == 0xFFFFFFFFu) continue;
            const unsigned w2 = wave_min_u32(k1 == w1 ? k2 : k1);
            const int bestDist1 = (int)(w1 >> 16), bestDist2 = w2 == 0xFFFFFFFFu ? 256 : (int)(w2 >> 16);
            if (bestDist1 < TH_LOW && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {     // :600-602
                const int kbest = (int)(w1 & 0xFFFFu);
                if ((kbest & 63) == lane) {
                    const int idx2 = (int)feat2[b0 + kbest];
                    m12[row + idx1] = idx2;                                   // :604-605
                    matched2[row + idx2] = 1;
                    bins[row + idx1] = (int8_t)(checkOrientation ? pg_rot_bin(B.fv.K[(int64_t)f1 * cap + idx1].angle,
                                                                              B.fv.K[(int64_t)f2 * cap + idx2].angle) : -1);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the next feature's scan reads matched2 from other lanes
            }
        }
    }
}

// after the nodes: the count and the rotation histogram (:636-654) of pair p over KF1's features
__global__ __launch_bounds__(64) void k_bow_keyframes_finish(PgKfBowBatch B, int checkOrientation, int32_t* __restrict__ m12,
                                                             const int8_t* __restrict__ bins, int32_t* __restrict__ nmatchesOut)
{
    const int p = blockIdx.x, cap = B.fv.cap, lane = threadIdx.x;
    const int n1 = min(max(B.fv.n[B.kf1[p]], 0), cap);
    m12 += (int64_t)p * cap; bins += (int64_t)p * cap;
    int nmatches = 0;
    for (int i = lane; i < n1; i += 64) nmatches += m12[i] >= 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nmatches += __shfl_xor(nmatches, d);
    if (checkOrientation) {
        __shared__ int hist[64];
        hist[lane] = 0;
        __syncthreads();
        for (int i = lane; i < n1; i += 64) { const int bb = bins[i]; if (bb >= 0 && m12[i] >= 0) atomicAdd(&hist[bb & 63], 1); }
        __syncthreads();
        const int h = hist[lane];
        int ind1, ind2, ind3;
        pg_three_maxima([&](int i) { return __shfl(h, i); }, ind1, ind2, ind3);
        int removed = 0;
        for (int i = lane; i < n1; i += 64) {
            const int bb = bins[i];
            if (bb >= 0 && bb != ind1 && bb != ind2 && bb != ind3 && m12[i] >= 0) { m12[i] = -1; removed++; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) removed += __shfl_xor(removed, d);
        nmatches -= removed;
    }
    if (lane == 0) nmatchesOut[p] = nmatches;
}

static bool pg_loop_tables(pgorb_ctx* c, PgLoopBatch& B, float min_x, float max_x, float min_y, float max_y, float th)
{
    pgorb_scale_tables(c, B.sf, nullptr, nullptr, nullptr);
    B.nlevels = pgorb_levels(c);
    B.logSf = pgorb_log_scale_factor(c);
    B.th = th;
    B.invW = (float)PGORB_GRID_COLS / (max_x - min_x);                 // Frame.cc:216-217, copied by the KeyFrame
    B.invH = (float)PGORB_GRID_ROWS / (max_y - min_y);
    B.minX = (float)(int)min_x; B.maxX = (float)(int)max_x;            // KeyFrame's const int mnMinX .. mnMaxY
    B.minY = (float)(int)min_y; B.maxY = (float)(int)max_y;
    return B.nlevels > 0;
}

// offsets of 256-byte aligned arrays inside one block of the matchers' scratch arena; `o` ends as the block's size
struct PgLoopCarve {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; }
};

// the single calls' shared checks of the table, the slots and the queries; null = fine
static const char* pg_loop_check(int n, const int32_t* slots, int npoints, int nq, const int32_t* queries)
{
    for (int i = 0; slots && i < n; i++)
        if (slots[i] < -1 || slots[i] >= npoints) return "a slot's point index is out of range";
    for (int q = 0; q < nq; q++)
        if (queries[q] < 0 || queries[q] >= npoints) return "a query index is out of range";
    return nullptr;
}

extern "C" {

int pgorb_fuse_sim3_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                 const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf, int nprob,
                                 const pgorb_kf_pose* d_pose, float min_x, float max_x, float min_y, float max_y,
                                 const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
                                 const uint8_t* d_point_bad, int qcap, const int32_t* d_nq, const int32_t* d_queries, float th,
                                 int32_t* d_action, int32_t* d_replace_point, int32_t* d_best_idx, int32_t* d_best_dist,
                                 int32_t* d_kf_point_out, int32_t* d_nfused, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || nprob < 0 || npoints < 0 || qcap < 1 ||
        !(max_x > min_x) || !(max_y > min_y) || !(th > 0.0f) ||
        (nprob && (!d_kf || !d_pose || !d_nq || !d_queries || !d_action || !d_replace_point || !d_nfused)) ||
        (npoints && (!d_points || !d_point_desc)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_fuse_sim3_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!nprob) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    PgLoopBatch B = {d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_kf, d_pose, d_kf_point, 0, npoints, d_points, d_point_desc,
                     d_point_bad, qcap, d_nq, d_queries};
    if (!pg_loop_tables(c, B, min_x, max_x, min_y, max_y, th)) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    const size_t rq = (size_t)nprob * qcap * 4, rs = (size_t)nprob * cap * 4, rf = (size_t)nprob * std::max(npoints, 1);
    PgLoopCarve cv;
    const size_t oBest = cv.take(rq), oDist = cv.take(rq), oAct = cv.take(rq), oHead = cv.take(rs), oFound = cv.take(rf);
    void* scr;
    int rc = pg_ctx_scratch(c, cv.o, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    int32_t* best = (int32_t*)(b + oBest); int32_t* dist = (int32_t*)(b + oDist); int32_t* act = (int32_t*)(b + oAct);
    int32_t* head = (int32_t*)(b + oHead);
    B.found = b + oFound;
    if (hipMemsetAsync(B.found, 0, rf, s) != hipSuccess || hipMemsetAsync(head, 0x7F, rs, s) != hipSuccess ||
        hipMemsetAsync(d_nfused, 0, (size_t)nprob * 4, s) != hipSuccess)
        return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    const unsigned gs = (unsigned)((cap + 255) / 256), gq = (unsigned)((qcap + 255) / 256);
    if (d_kf_point && npoints) hipLaunchKernelGGL(k_loop_mark, dim3(gs, (unsigned)nprob), dim3(256), 0, s, B);
    hipLaunchKernelGGL(k_fs3_match, dim3(gq, (unsigned)nprob), dim3(256), 0, s, B, best, dist, act, head);
    hipLaunchKernelGGL(k_fs3_resolve, dim3(std::max(gs, gq), (unsigned)nprob), dim3(256), 0, s, B, best, dist, act, head, d_action,
                       d_replace_point, d_best_idx, d_best_dist, d_kf_point_out, d_nfused);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_fs3_match / k_fs3_resolve launch failed");
    return pg_ctx_scratch_done(c, s);
}

int pgorb_search_by_projection_sim3_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                                 int cap, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf,
                                                 int nprob, const pgorb_kf_pose* d_pose, float min_x, float max_x, float min_y,
                                                 float max_y, const int32_t* d_matched_in, int npoints, const pgorb_map_point* d_points,
                                                 const uint8_t* d_point_desc, const uint8_t* d_point_bad, int qcap, const int32_t* d_nq,
                                                 const int32_t* d_queries, int th, int32_t* d_assigned, int32_t* d_matched_out,
                                                 int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || nprob < 0 || npoints < 0 || qcap < 1 ||
        !(max_x > min_x) || !(max_y > min_y) || th < 1 ||
        (nprob && (!d_kf || !d_pose || !d_nq || !d_queries || !d_assigned || !d_nmatches)) ||
        (npoints && (!d_points || !d_point_desc)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_projection_sim3_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!nprob) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    PgLoopBatch B = {d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_kf, d_pose, d_matched_in, 1, npoints, d_points, d_point_desc,
                     d_point_bad, qcap, d_nq, d_queries};
    if (!pg_loop_tables(c, B, min_x, max_x, min_y, max_y, (float)th)) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    const size_t lds = (size_t)cap * 5;
    if (!pg_raise_lds<k_ps3_decide>(c, lds)) return pg_ctx_fail(c, PGORB_E_LIMIT, "SearchByProjection state exceeds the LDS");
    const size_t rq = (size_t)nprob * qcap * 4, rf = (size_t)nprob * std::max(npoints, 1);
    PgLoopCarve cv;
    const size_t oLists = cv.take(rq * LOOP_K), oCnt = cv.take((size_t)nprob * qcap * sizeof(uint16_t)), oA = cv.take(rq), oB = cv.take(rq), oDec = cv.take(rq),
                 oFound = cv.take(rf);
    void* scr;
    int rc = pg_ctx_scratch(c, cv.o, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    B.found = b + oFound;
    if (hipMemsetAsync(B.found, 0, rf, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (d_matched_in && npoints) hipLaunchKernelGGL(k_loop_mark, dim3((unsigned)((cap + 255) / 256), (unsigned)nprob), dim3(256), 0, s, B);
    hipLaunchKernelGGL(k_ps3_lists, dim3((unsigned)((qcap + 255) / 256), (unsigned)nprob), dim3(256), 0, s, B, (uint32_t*)(b + oLists),
                       (uint16_t*)(b + oCnt));
    hipLaunchKernelGGL(k_ps3_decide, dim3((unsigned)nprob), dim3(LOOP_T), lds, s, B, (const uint32_t*)(b + oLists),
                       (const uint16_t*)(b + oCnt), (int32_t*)(b + oA), (int32_t*)(b + oB), (int32_t*)(b + oDec), d_assigned,
                       d_matched_out, d_nmatches);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_ps3_lists / k_ps3_decide launch failed");
    return pg_ctx_scratch_done(c, s);
}


int pgorb_search_by_bow_keyframes_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                               const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat,
                                               const int32_t* d_nfv, const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs,
                                               const uint8_t* d_point_valid1, const uint8_t* d_point_valid2, float nnratio,
                                               int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv || npairs < 0 ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_point_valid1 || !d_point_valid2 || !d_matches12 || !d_nmatches)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow_keyframes_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const size_t rb = (size_t)npairs * cap;                                  // the rotation bins (i8) and vbMatched2 (u8) of every pair
    PgLoopCarve cv;
    const size_t oBins = cv.take(rb), oM2 = cv.take(rb);
    void* scr;
    int rc = pg_ctx_scratch(c, cv.o, s, &scr);
    if (rc) return rc;
    int8_t* bins = (int8_t*)scr + oBins;
    uint8_t* matched2 = (uint8_t*)scr + oM2;
    if (hipMemsetAsync(d_matches12, 0xFF, rb * 4, s) != hipSuccess || hipMemsetAsync(bins, 0xFF, rb, s) != hipSuccess ||
        hipMemsetAsync(matched2, 0, rb, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    const PgKfBowBatch B = {{d_kps, d_desc, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv}, d_pair_kf1, d_pair_kf2, d_point_valid1,
                            d_point_valid2};
    hipLaunchKernelGGL(k_bow_keyframes, dim3(KFBOW_WAVES, (unsigned)npairs), dim3(64), 0, s, B, nnratio, check_orientation, d_matches12,
                       bins, matched2);
    hipLaunchKernelGGL(k_bow_keyframes_finish, dim3((unsigned)npairs), dim3(64), 0, s, B, check_orientation, d_matches12,
                       (const int8_t*)bins, d_nmatches);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_bow_keyframes launch failed");
    return pg_ctx_scratch_done(c, s);
}

// single pair through host buffers: a two-frame batch (KF1 = frame 0, KF2 = frame 1); the FeatureVectors are checked here
int pgorb_search_by_bow_keyframes(pgorb_ctx* c, const uint8_t* desc1, const float* angle1, const uint8_t* point_valid1, int n1,
                                  const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1,
                                  const uint8_t* desc2, const float* angle2, const uint8_t* point_valid2, int n2,
                                  const uint32_t* fv2_node, const int32_t* fv2_start, const uint32_t* fv2_feat, int nfv2,
                                  float nnratio, int check_orientation, int32_t* matches12)
{
    if (!c) return PGORB_E_ARG;
    if (n1 < 0 || n2 < 0 || nfv1 < 0 || nfv2 < 0 || (n1 && !matches12) || (n1 && (!desc1 || !angle1 || !point_valid1)) ||
        (n2 && (!desc2 || !angle2 || !point_valid2)) || (nfv1 && (!fv1_node || !fv1_start || !fv1_feat)) ||
        (nfv2 && (!fv2_node || !fv2_start || !fv2_feat)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow_keyframes");
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (!n1 || !n2 || !nfv1 || !nfv2) return 0;
    if (n1 > 16000 || n2 > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (!pg_fv_ok(fv1_start, fv1_feat, nfv1, n1) || !pg_fv_ok(fv2_start, fv2_feat, nfv2, n2))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: FeatureVector names more features than the key frame has");
    for (int a = 1; a < nfv1; a++) if (!(fv1_node[a - 1] < fv1_node[a])) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: node ids must ascend");
    for (int a = 1; a < nfv2; a++) if (!(fv2_node[a - 1] < fv2_node[a])) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: node ids must ascend");
    const PgFvFrame f[2] = {{nullptr, angle1, desc1, point_valid1, n1, fv1_node, fv1_start, fv1_feat, nfv1},
                            {nullptr, angle2, desc2, point_valid2, n2, fv2_node, fv2_start, fv2_feat, nfv2}};
    PgHostCall hc(c);
    const PgFvPack pk(hc, f, 2);
    const size_t oM = hc.region(PG_DOWN, (size_t)pk.cap * 4), oNM = hc.region(PG_DOWN, 4);
    int rc = hc.begin();
    if (rc) return rc;
    pk.pack(hc, f);
    if ((rc = hc.run([&] {
            return pgorb_search_by_bow_keyframes_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), pk.cap,
                                                              hc.dev<uint32_t>(pk.FN), hc.dev<int32_t>(pk.FS), hc.dev<uint32_t>(pk.FF),
                                                              hc.dev<int32_t>(pk.NF), hc.dev<int32_t>(pk.P), hc.dev<int32_t>(pk.P) + 1, 1,
                                                              hc.dev(pk.H), hc.dev(pk.H) + pk.cap, nnratio, check_orientation,
                                                              hc.dev<int32_t>(oM), hc.dev<int32_t>(oNM), nullptr); }))) return rc;
    memcpy(matches12, hc.host(oM), (size_t)n1 * 4);
    return *hc.host<int32_t>(oNM);
}

int pgorb_search_by_sim3_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                      const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_kf1,
                                      const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, float min_x, float max_x,
                                      float min_y, float max_y, const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points,
                                      const uint8_t* d_point_desc, const uint8_t* d_point_bad, const pgorb_sim3* d_sim3,
                                      const uint8_t* d_already1, const uint8_t* d_already2, float th, int32_t* d_match12,
                                      int32_t* d_nfound, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || npairs < 0 || npoints < 0 ||
        !(max_x > min_x) || !(max_y > min_y) || !(th > 0.0f) ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_pose || !d_sim3 || !d_match12 || !d_nfound)) ||
        (npoints && (!d_points || !d_point_desc)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_sim3_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    PgLoopBatch B = {d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, nullptr, d_pose, d_kf_point, 0, npoints, d_points, d_point_desc,
                     d_point_bad, 0, nullptr, nullptr};
    if (!pg_loop_tables(c, B, min_x, max_x, min_y, max_y, th)) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    const PgSim3Batch E = {d_pair_kf1, d_pair_kf2, d_sim3, d_already1, d_already2};
    const size_t rs = (size_t)npairs * cap * sizeof(int32_t);
    PgLoopCarve cv;
    const size_t o1 = cv.take(rs), o2 = cv.take(rs);
    void* scr;
    int rc = pg_ctx_scratch(c, cv.o, s, &scr);
    if (rc) return rc;
    int32_t* m1 = (int32_t*)((uint8_t*)scr + o1); int32_t* m2 = (int32_t*)((uint8_t*)scr + o2);
    if (hipMemsetAsync(d_nfound, 0, (size_t)npairs * 4, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    const unsigned gs = (unsigned)((cap + 255) / 256);
    hipLaunchKernelGGL(k_s3_match, dim3(gs, (unsigned)npairs, 2), dim3(256), 0, s, B, E, m1, m2);
    hipLaunchKernelGGL(k_s3_agree, dim3(gs, (unsigned)npairs), dim3(256), 0, s, B, E, m1, m2, d_match12, d_nfound);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_s3_match / k_s3_agree launch failed");
    return pg_ctx_scratch_done(c, s);
}

// one pair through host buffers: a two-frame, one-pair batch; the inputs are checked here
int pgorb_search_by_sim3(pgorb_ctx* c, const pgorb_keypoint* kps1, const uint8_t* desc1, int n1, const pgorb_kf_pose* pose1,
                         const int32_t* kf_point1, const uint8_t* already1, const pgorb_keypoint* kps2, const uint8_t* desc2, int n2,
                         const pgorb_kf_pose* pose2, const int32_t* kf_point2, const uint8_t* already2, float min_x, float max_x,
                         float min_y, float max_y, int npoints, const pgorb_map_point* points, const uint8_t* point_desc,
                         const uint8_t* point_bad, const pgorb_sim3* sim3, float th, int32_t* match12)
{
    if (!c) return PGORB_E_ARG;
    if (n1 < 0 || n2 < 0 || npoints < 0 || !pose1 || !pose2 || !sim3 || !(max_x > min_x) || !(max_y > min_y) || !(th > 0.0f) ||
        (n1 && (!kps1 || !desc1 || !match12)) || (n2 && (!kps2 || !desc2)) || (npoints && (!points || !point_desc)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_sim3");
    if (n1 > 16000 || n2 > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    const char* bad = pg_loop_check(n1, kf_point1, npoints, 0, nullptr);
    if (!bad) bad = pg_loop_check(n2, kf_point2, npoints, 0, nullptr);
    if (bad) return pg_ctx_fail(c, PGORB_E_ARG, bad);
    const int cap = std::max(std::max(n1, n2), 1), np = std::max(npoints, 1);
    PgHostCall hc(c);
    const size_t kb = sizeof(pgorb_keypoint);
    const size_t oN = hc.region(PG_UP, 8), oK = hc.region(PG_UP, (size_t)2 * cap * kb), oD = hc.region(PG_UP, (size_t)2 * cap * 32),
                 oS = hc.region(PG_UP, (size_t)2 * cap * 4), oPose = hc.region(PG_UP, 2 * sizeof(pgorb_kf_pose)), oF = hc.region(PG_UP, 8),
                 oP = hc.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)), oPD = hc.region(PG_UP, (size_t)np * 32),
                 oB = hc.region(PG_UP, np), oX = hc.region(PG_UP, sizeof(pgorb_sim3)), oA1 = hc.region(PG_UP, cap), oA2 = hc.region(PG_UP, cap),
                 oM = hc.region(PG_DOWN, (size_t)cap * 4), oNF = hc.region(PG_DOWN, 4),
                 oGS = hc.region(PG_DEV, (size_t)2 * (PGORB_GRID_CELLS + 1) * 4), oGI = hc.region(PG_DEV, (size_t)2 * cap * 4);
    int rc = hc.begin();
    if (rc) return rc;
    const int32_t cnt[2] = {n1, n2}, fr[2] = {0, 1};
    hc.put(oN, cnt, 8);
    hc.put(oF, fr, 8);
    hc.put(oK, kps1, (size_t)n1 * kb, 0, (size_t)cap * kb);
    hc.put(oK, kps2, (size_t)n2 * kb, (size_t)cap * kb, (size_t)cap * kb);
    hc.put(oD, desc1, (size_t)n1 * 32, 0, (size_t)cap * 32);
    hc.put(oD, desc2, (size_t)n2 * 32, (size_t)cap * 32, (size_t)cap * 32);
    memset(hc.host(oS), 0xFF, (size_t)2 * cap * 4);
    if (kf_point1) memcpy(hc.host(oS), kf_point1, (size_t)n1 * 4);
    if (kf_point2) memcpy(hc.host(oS) + (size_t)cap * 4, kf_point2, (size_t)n2 * 4);
    hc.put(oPose, pose1, sizeof(pgorb_kf_pose));
    hc.put(oPose, pose2, sizeof(pgorb_kf_pose), sizeof(pgorb_kf_pose));
    hc.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point));
    hc.put(oPD, point_desc, (size_t)npoints * 32);
    hc.put(oB, point_bad, npoints, 0, npoints);
    hc.put(oX, sim3, sizeof(pgorb_sim3));
    hc.put(oA1, already1, n1, 0, cap);
    hc.put(oA2, already2, n2, 0, cap);
    if ((rc = hc.run([&] {
            int r = pgorb_frame_grid_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev<int32_t>(oN), 2, cap, min_x, max_x, min_y, max_y,
                                                  hc.dev<int32_t>(oGS), hc.dev<int32_t>(oGI), nullptr);
            return r ? r : pgorb_search_by_sim3_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev(oD), hc.dev<int32_t>(oN), cap,
                                                             hc.dev<int32_t>(oGS), hc.dev<int32_t>(oGI), hc.dev<int32_t>(oF),
                                                             hc.dev<int32_t>(oF) + 1, 1, hc.dev<pgorb_kf_pose>(oPose), min_x, max_x, min_y,
                                                             max_y, hc.dev<int32_t>(oS), npoints, hc.dev<pgorb_map_point>(oP), hc.dev(oPD),
                                                             hc.dev(oB), hc.dev<pgorb_sim3>(oX), hc.dev(oA1), hc.dev(oA2), th,
                                                             hc.dev<int32_t>(oM), hc.dev<int32_t>(oNF), nullptr); }))) return rc;
    memcpy(match12, hc.host(oM), (size_t)n1 * 4);
    return *hc.host<int32_t>(oNF);
}

// One key frame through host buffers: a one-problem batch; the inputs are checked here.  `fuse` selects the routine: the slots are
// kf_point (Fuse) or matched_in (SearchByProjection), out0 / out1 = action / replace_point or assigned / (unused).
static int pg_loop_single(pgorb_ctx* c, bool fuse, const char* name, const pgorb_keypoint* kps, const uint8_t* desc, int n,
                          const pgorb_kf_pose* pose, float min_x, float max_x, float min_y, float max_y, const int32_t* slots, int npoints,
                          const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad, int nq,
                          const int32_t* queries, float th, int32_t* out0, int32_t* out1, int32_t* best_idx, int32_t* best_dist,
                          int32_t* slots_out)
{
    if (!c) return PGORB_E_ARG;
    if (n < 0 || npoints < 0 || nq < 0 || !pose || !(max_x > min_x) || !(max_y > min_y) || !(th > 0.0f) || (n && (!kps || !desc)) ||
        (npoints && (!points || !point_desc)) || (nq && (!queries || !out0)) || (fuse && nq && !out1) || (!fuse && n && !out0))
        return pg_ctx_fail(c, PGORB_E_ARG, name);
    if (n > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (const char* bad = pg_loop_check(n, slots, npoints, nq, queries)) return pg_ctx_fail(c, PGORB_E_ARG, bad);
    const int cap = std::max(n, 1), np = std::max(npoints, 1), qc = std::max(nq, 1);
    PgHostCall hc(c);
    const size_t kb = sizeof(pgorb_keypoint);
    const size_t oN = hc.region(PG_UP, 8), oK = hc.region(PG_UP, (size_t)cap * kb), oD = hc.region(PG_UP, (size_t)cap * 32),
                 oS = hc.region(PG_UP, (size_t)cap * 4), oPose = hc.region(PG_UP, sizeof(pgorb_kf_pose)), oF = hc.region(PG_UP, 4),
                 oP = hc.region(PG_UP, (size_t)np * sizeof(pgorb_map_point)), oPD = hc.region(PG_UP, (size_t)np * 32),
                 oB = hc.region(PG_UP, np), oQ = hc.region(PG_UP, (size_t)qc * 4),
                 oA = hc.region(PG_DOWN, (size_t)std::max(qc, cap) * 4), oR = hc.region(PG_DOWN, (size_t)qc * 4),
                 oBI = hc.region(PG_DOWN, (size_t)qc * 4), oBD = hc.region(PG_DOWN, (size_t)qc * 4),
                 oSO = hc.region(PG_DOWN, (size_t)cap * 4), oNF = hc.region(PG_DOWN, 4),
                 oGS = hc.region(PG_DEV, (size_t)(PGORB_GRID_CELLS + 1) * 4), oGI = hc.region(PG_DEV, (size_t)cap * 4);
    int rc = hc.begin();
    if (rc) return rc;
    const int32_t cnt[2] = {n, nq};
    hc.put(oN, cnt, 8);
    hc.put(oK, kps, (size_t)n * kb, 0, (size_t)cap * kb);
    hc.put(oD, desc, (size_t)n * 32, 0, (size_t)cap * 32);
    if (slots) hc.put(oS, slots, (size_t)n * 4);
    else memset(hc.host(oS), 0xFF, (size_t)cap * 4);
    hc.put(oPose, pose, sizeof(pgorb_kf_pose));
    hc.put(oF, nullptr, 0, 0, 4);
    hc.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point));
    hc.put(oPD, point_desc, (size_t)npoints * 32);
    hc.put(oB, point_bad, npoints, 0, npoints);
    hc.put(oQ, queries, (size_t)nq * 4);
    if ((rc = hc.run([&] {
            int r = pgorb_frame_grid_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev<int32_t>(oN), 1, cap, min_x, max_x, min_y, max_y,
                                                  hc.dev<int32_t>(oGS), hc.dev<int32_t>(oGI), nullptr);
            if (r) return r;
            if (fuse)
                return pgorb_fuse_sim3_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev(oD), hc.dev<int32_t>(oN), cap, hc.dev<int32_t>(oGS),
                                                    hc.dev<int32_t>(oGI), hc.dev<int32_t>(oF), 1, hc.dev<pgorb_kf_pose>(oPose), min_x, max_x,
                                                    min_y, max_y, hc.dev<int32_t>(oS), npoints, hc.dev<pgorb_map_point>(oP), hc.dev(oPD),
                                                    hc.dev(oB), qc, hc.dev<int32_t>(oN) + 1, hc.dev<int32_t>(oQ), th, hc.dev<int32_t>(oA),
                                                    hc.dev<int32_t>(oR), hc.dev<int32_t>(oBI), hc.dev<int32_t>(oBD), hc.dev<int32_t>(oSO),
                                                    hc.dev<int32_t>(oNF), nullptr);
            return pgorb_search_by_projection_sim3_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev(oD), hc.dev<int32_t>(oN), cap,
                                                                hc.dev<int32_t>(oGS), hc.dev<int32_t>(oGI), hc.dev<int32_t>(oF), 1,
                                                                hc.dev<pgorb_kf_pose>(oPose), min_x, max_x, min_y, max_y, hc.dev<int32_t>(oS),
                                                                npoints, hc.dev<pgorb_map_point>(oP), hc.dev(oPD), hc.dev(oB), qc,
                                                                hc.dev<int32_t>(oN) + 1, hc.dev<int32_t>(oQ), (int)th, hc.dev<int32_t>(oA),
                                                                hc.dev<int32_t>(oSO), hc.dev<int32_t>(oNF), nullptr); }))) return rc;
    if (fuse) {
        memcpy(out0, hc.host(oA), (size_t)nq * 4);
        memcpy(out1, hc.host(oR), (size_t)nq * 4);
        if (best_idx) memcpy(best_idx, hc.host(oBI), (size_t)nq * 4);
        if (best_dist) memcpy(best_dist, hc.host(oBD), (size_t)nq * 4);
    } else {
        memcpy(out0, hc.host(oA), (size_t)n * 4);
    }
    if (slots_out) memcpy(slots_out, hc.host(oSO), (size_t)n * 4);
    return *hc.host<int32_t>(oNF);
}

int pgorb_fuse_sim3(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* pose,
                    float min_x, float max_x, float min_y, float max_y, const int32_t* kf_point, int npoints,
                    const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad, int nq, const int32_t* queries,
                    float th, int32_t* action, int32_t* replace_point, int32_t* best_idx, int32_t* best_dist, int32_t* kf_point_out)
{
    return pg_loop_single(c, true, "bad argument to pgorb_fuse_sim3", kps, desc, n, pose, min_x, max_x, min_y, max_y, kf_point, npoints,
                          points, point_desc, point_bad, nq, queries, th, action, replace_point, best_idx, best_dist, kf_point_out);
}

int pgorb_search_by_projection_sim3(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* pose,
                                    float min_x, float max_x, float min_y, float max_y, const int32_t* matched_in, int npoints,
                                    const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad, int nq,
                                    const int32_t* queries, int th, int32_t* assigned, int32_t* matched_out)
{
    return pg_loop_single(c, false, "bad argument to pgorb_search_by_projection_sim3", kps, desc, n, pose, min_x, max_x, min_y, max_y,
                          matched_in, npoints, points, point_desc, point_bad, nq, queries, (float)th, assigned, nullptr, nullptr,
                          nullptr, matched_out);
}

}  // extern "C"
