// loop.hip -- loop closing's three projection matchers on gfx950, monocular: SearchBySim3 and the two that take Scw.  (The fourth
// matcher of loop closing, SearchByBoW(KF, KF), is a BoW-node matcher: node_match.hip.)
//
// Restates (thirdparty/orb-slam2):
//   ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)   src/ORBmatcher.cc:292-405
//   ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)            src/ORBmatcher.cc:981-1104
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)        src/ORBmatcher.cc:1106-1330
//   KeyFrame::GetFeaturesInArea / IsInImage / GetMapPoints                     src/KeyFrame.cc:672-716, 338-351
//
// The Scw forms both project a list of map points through the decomposed Scw (the caller's pgorb_kf_pose) with Fuse's front part
// (kf_window.h: the image, depth and viewing-angle tests, PredictScale) and scan the key frame's search window in the reference's
// (ix, iy, insertion) order for the first smallest descriptor distance among octaves [level - 1, level] (kf_scan).  There is no
// chi-square test.  spAlreadyFound is the state
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
// Every float operation follows the reference's cv::Mat arithmetic under the readings of DESIGN.md section 4.
#include "kf_window.h"

#define LOOP_T 1024
#define LOOP_K 64                           // candidates a query's list holds; more: the query is evaluated in place
#define LOOP_OVER 0xFFFF
#define LOOP_NONE 0x7FFFFFFF

struct PgLoopBatch {
    PgKfBatch kb;
    const int32_t* kf;
    const int32_t* slots;                  // Fuse: kf_point [nframes][cap]; SearchByProjection: matched_in [nprob][cap]; or null
    int slotsPerProblem;                   // 1: slots rows go by problem, 0: by key frame
    int qcap; const int32_t* nq; const int32_t* queries;
    uint8_t* found;                        // [nprob][npoints] spAlreadyFound
};

__device__ __forceinline__ int64_t loop_slot_row(const PgLoopBatch& B, int p, int f) { return (int64_t)(B.slotsPerProblem ? p : f) * B.kb.cap; }
// the occupant of slot s on entry: a table index, or -1 (out of range counts as NULL)
__device__ __forceinline__ int loop_occupant(const PgLoopBatch& B, int64_t row, int s)
{
    if (!B.slots) return -1;
    const int o = B.slots[row + s];
    return (o >= 0 && o < B.kb.npoints) ? o : -1;
}

// spAlreadyFound of every problem (the mask is zeroed before)
__global__ __launch_bounds__(256) void k_loop_mark(PgLoopBatch B)
{
    const int p = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, f = B.kf[p];
    const int n = min(max(B.kb.n[f], 0), B.kb.cap);
    if (s >= n) return;
    const int o = loop_occupant(B, loop_slot_row(B, p, f), s);
    if (o >= 0) B.found[(int64_t)p * B.kb.npoints + o] = 1;
}

// :316-367 / :1006-1058 for query point mp of problem p: the skips (out of range, bad, in spAlreadyFound), then the front part
__device__ __forceinline__ bool loop_query(const PgLoopBatch& B, int p, int f, int mp, KfQuery& Q)
{
    const PgKfBatch& W = B.kb;
    if (mp < 0 || mp >= W.npoints || (W.pbad && W.pbad[mp]) || B.found[(int64_t)p * W.npoints + mp]) return false;
    return kf_point_query(W, f, mp, Q);
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
    KfQuery Q;
    if (loop_query(B, p, f, mp, Q)) {
        int d1 = 256, i1 = -1;
        const bool any = kf_scan(B.kb, f, mp, Q, [](int, const pgorb_keypoint&) { return false; },
                                 [&](int idx, int d) { if (d < d1) { d1 = d; i1 = idx; } });      // :1078-1082
        if (any) {
            bi = i1; bd = d1;
            a = PGORB_FUSE_NO_MATCH;
            if (d1 <= TH_LOW) { a = PGORB_FUSE_ADDED; atomicMin(&head[(int64_t)p * B.kb.cap + i1], q); }   // provisional: k_fs3_resolve
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
    const int nq = min(max(B.nq[p], 0), B.qcap), n = min(max(B.kb.n[f], 0), B.kb.cap);
    const int64_t rowQ = (int64_t)p * B.qcap, rowS = (int64_t)p * B.kb.cap, rowIn = loop_slot_row(B, p, f);
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
                if (B.kb.pbad && B.kb.pbad[o]) a = PGORB_FUSE_KF_POINT_BAD;
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
    KfQuery Q;
    if (loop_query(B, p, f, mp, Q)) {
        uint32_t* L = lists + qi * LOOP_K;
        kf_scan(B.kb, f, mp, Q, [&](int idx, const pgorb_keypoint&) { return loop_occupant(B, rowIn, idx) >= 0; },   // :377 on the entry state
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
    const int p = blockIdx.x, tid = threadIdx.x, f = B.kf[p], cap = B.kb.cap;
    const int n = min(max(B.kb.n[f], 0), cap), nq = min(max(B.nq[p], 0), B.qcap);
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
                    KfQuery Q;
                    int d1 = 256, i1 = -1;
                    if (loop_query(B, p, f, mp, Q))
                        kf_scan(B.kb, f, mp, Q, [&](int idx, const pgorb_keypoint&) { return taken[idx] != 0; },
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
    const PgKfBatch& W = B.kb;
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, dir = blockIdx.z;
    const int f1 = E.kf1[p], f2 = E.kf2[p];
    const int fs = dir ? f2 : f1, ft = dir ? f1 : f2;                                    // source and target key frame
    const int ns = min(max(W.n[fs], 0), W.cap);
    if (i >= ns) return;
    int32_t* out = (dir ? m2 : m1) + (int64_t)p * W.cap;
    const uint8_t* already = dir ? E.already2 : E.already1;
    int res = -1;
    const int mp = loop_occupant(B, (int64_t)fs * W.cap, i);
    if (mp >= 0 && !(already && already[(int64_t)p * W.cap + i]) && !(W.pbad && W.pbad[mp])) {
        const pgorb_map_point P = W.pts[mp];
        const pgorb_sim3& S = E.sim3[p];
        const float* M = dir ? S.sR12 : S.sR21;
        const float* t = dir ? S.t12 : S.t21;
        // p3Dc = Rw*p3Dw + tw, then sR*p3Dc + t: gemm's small-matrix path twice, the translation as C
        float a[3], b[3];
        kf_to_camera(W.pose[fs], P.pos, a);
#pragma unroll
        for (int r = 0; r < 3; r++) b[r] = kf_row(M + 3 * r, t[r], a);
        KfQuery Q;
        // pKF1's fx, fy, cx, cy in both directions; cv::norm of the camera-frame vector, no viewing-angle test
        if (kf_query(W, W.pose[f1], P, b, [&](float& dist3D) { dist3D = cnm_f(cnm_normd(b[0], b[1], b[2])); return kf_depth_ok(P, dist3D); }, Q)) {
            int d1 = 0x7FFFFFFF, i1 = -1;
            kf_scan(W, ft, mp, Q, [](int, const pgorb_keypoint&) { return false; }, [&](int idx, int d) { if (d < d1) { d1 = d; i1 = idx; } });
            if (d1 <= TH_HIGH) res = i1;
        }
    }
    out[i] = res;
}

__global__ __launch_bounds__(256) void k_s3_agree(PgLoopBatch B, PgSim3Batch E, const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                  int32_t* __restrict__ match12, int32_t* __restrict__ nfound)
{
    const int p = blockIdx.y, i1 = blockIdx.x * 256 + threadIdx.x;
    const int n1 = min(max(B.kb.n[E.kf1[p]], 0), B.kb.cap), n2 = min(max(B.kb.n[E.kf2[p]], 0), B.kb.cap);
    bool ok = false;
    if (i1 < n1) {
        const int idx2 = m1[(int64_t)p * B.kb.cap + i1];
        ok = idx2 >= 0 && idx2 < n2 && m2[(int64_t)p * B.kb.cap + idx2] == i1;            // :1314-1327
        match12[(int64_t)p * B.kb.cap + i1] = ok ? idx2 : -1;
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nfound[p], __popcll(m));
}

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
    PgLoopBatch B = {{d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_pose, npoints, d_points, d_point_desc, d_point_bad},
                     d_kf, d_kf_point, 0, qcap, d_nq, d_queries};
    int rc;
    if (pg_kf_begin(c, "bad argument to pgorb_fuse_sim3_batch_device",
                    qcap >= 1 && (!nprob || (d_kf && d_nq && d_queries && d_action && d_replace_point && d_nfused)), B.kb, nprob,
                    min_x, max_x, min_y, max_y, th, rc)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const size_t rq = (size_t)nprob * qcap * 4, rs = (size_t)nprob * cap * 4, rf = (size_t)nprob * std::max(npoints, 1);
    PgCarve cv;
    const size_t oBest = cv.take(rq), oDist = cv.take(rq), oAct = cv.take(rq), oHead = cv.take(rs), oFound = cv.take(rf);
    void* scr;
    if ((rc = pg_ctx_scratch(c, cv.o, s, &scr))) return rc;
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
    PgLoopBatch B = {{d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_pose, npoints, d_points, d_point_desc, d_point_bad},
                     d_kf, d_matched_in, 1, qcap, d_nq, d_queries};
    int rc;
    if (pg_kf_begin(c, "bad argument to pgorb_search_by_projection_sim3_batch_device",
                    qcap >= 1 && (!nprob || (d_kf && d_nq && d_queries && d_assigned && d_nmatches)), B.kb, nprob, min_x, max_x, min_y,
                    max_y, (float)th, rc)) return rc;                       // (an int th below 1 fails the shared th > 0)
    const hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)cap * 5;
    if (!pg_raise_lds<k_ps3_decide>(c, lds)) return pg_ctx_fail(c, PGORB_E_LIMIT, "SearchByProjection state exceeds the LDS");
    const size_t rq = (size_t)nprob * qcap * 4, rf = (size_t)nprob * std::max(npoints, 1);
    PgCarve cv;
    const size_t oLists = cv.take(rq * LOOP_K), oCnt = cv.take((size_t)nprob * qcap * sizeof(uint16_t)), oA = cv.take(rq), oB = cv.take(rq), oDec = cv.take(rq),
                 oFound = cv.take(rf);
    void* scr;
    if ((rc = pg_ctx_scratch(c, cv.o, s, &scr))) return rc;
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

int pgorb_search_by_sim3_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                      const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_kf1,
                                      const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, float min_x, float max_x,
                                      float min_y, float max_y, const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points,
                                      const uint8_t* d_point_desc, const uint8_t* d_point_bad, const pgorb_sim3* d_sim3,
                                      const uint8_t* d_already1, const uint8_t* d_already2, float th, int32_t* d_match12,
                                      int32_t* d_nfound, void* stream)
{
    PgLoopBatch B = {{d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_pose, npoints, d_points, d_point_desc, d_point_bad},
                     nullptr, d_kf_point, 0, 0, nullptr, nullptr};
    int rc;
    if (pg_kf_begin(c, "bad argument to pgorb_search_by_sim3_batch_device",
                    !npairs || (d_pair_kf1 && d_pair_kf2 && d_sim3 && d_match12 && d_nfound), B.kb, npairs, min_x, max_x, min_y, max_y,
                    th, rc)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const PgSim3Batch E = {d_pair_kf1, d_pair_kf2, d_sim3, d_already1, d_already2};
    const size_t rs = (size_t)npairs * cap * sizeof(int32_t);
    PgCarve cv;
    const size_t o1 = cv.take(rs), o2 = cv.take(rs);
    void* scr;
    if ((rc = pg_ctx_scratch(c, cv.o, s, &scr))) return rc;
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
    const PgKfFrame f[2] = {{kps1, desc1, kf_point1, pose1, n1}, {kps2, desc2, kf_point2, pose2, n2}};
    PgHostCall hc(c);
    PgKfPack pk(hc, f, 2, npoints);
    const int cap = pk.cap;
    const size_t oX = hc.region(PG_UP, sizeof(pgorb_sim3)), oA1 = hc.region(PG_UP, cap), oA2 = hc.region(PG_UP, cap),
                 oM = hc.region(PG_DOWN, (size_t)cap * 4), oNF = hc.region(PG_DOWN, 4);
    pk.device(hc);
    int rc = hc.begin();
    if (rc) return rc;
    pk.pack(hc, f, points, point_desc, point_bad);
    hc.put(oX, sim3, sizeof(pgorb_sim3));
    hc.put(oA1, already1, n1, 0, cap);
    hc.put(oA2, already2, n2, 0, cap);
    if ((rc = hc.run([&] {
            const int r = pk.grid(c, hc, min_x, max_x, min_y, max_y);
            return r ? r : pgorb_search_by_sim3_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), cap,
                                                             hc.dev<int32_t>(pk.GS), hc.dev<int32_t>(pk.GI), hc.dev<int32_t>(pk.F),
                                                             hc.dev<int32_t>(pk.F) + 1, 1, hc.dev<pgorb_kf_pose>(pk.Pose), min_x, max_x, min_y,
                                                             max_y, hc.dev<int32_t>(pk.S), npoints, hc.dev<pgorb_map_point>(pk.P), hc.dev(pk.PD),
                                                             hc.dev(pk.B), hc.dev<pgorb_sim3>(oX), hc.dev(oA1), hc.dev(oA2), th,
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
    const int qc = std::max(nq, 1);
    const PgKfFrame f = {kps, desc, slots, pose, n};
    PgHostCall hc(c);
    PgKfPack pk(hc, &f, 1, npoints);
    const int cap = pk.cap;
    const size_t oNQ = hc.region(PG_UP, 4), oQ = hc.region(PG_UP, (size_t)qc * 4),
                 oA = hc.region(PG_DOWN, (size_t)std::max(qc, cap) * 4), oR = hc.region(PG_DOWN, (size_t)qc * 4),
                 oBI = hc.region(PG_DOWN, (size_t)qc * 4), oBD = hc.region(PG_DOWN, (size_t)qc * 4),
                 oSO = hc.region(PG_DOWN, (size_t)cap * 4), oNF = hc.region(PG_DOWN, 4);
    pk.device(hc);
    int rc = hc.begin();
    if (rc) return rc;
    pk.pack(hc, &f, points, point_desc, point_bad);
    hc.put(oNQ, &nq, 4);
    hc.put(oQ, queries, (size_t)nq * 4);
    if ((rc = hc.run([&] {
            const int r = pk.grid(c, hc, min_x, max_x, min_y, max_y);
            if (r) return r;
            if (fuse)
                return pgorb_fuse_sim3_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), cap, hc.dev<int32_t>(pk.GS),
                                                    hc.dev<int32_t>(pk.GI), hc.dev<int32_t>(pk.F), 1, hc.dev<pgorb_kf_pose>(pk.Pose), min_x, max_x,
                                                    min_y, max_y, hc.dev<int32_t>(pk.S), npoints, hc.dev<pgorb_map_point>(pk.P), hc.dev(pk.PD),
                                                    hc.dev(pk.B), qc, hc.dev<int32_t>(oNQ), hc.dev<int32_t>(oQ), th, hc.dev<int32_t>(oA),
                                                    hc.dev<int32_t>(oR), hc.dev<int32_t>(oBI), hc.dev<int32_t>(oBD), hc.dev<int32_t>(oSO),
                                                    hc.dev<int32_t>(oNF), nullptr);
            return pgorb_search_by_projection_sim3_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), cap,
                                                                hc.dev<int32_t>(pk.GS), hc.dev<int32_t>(pk.GI), hc.dev<int32_t>(pk.F), 1,
                                                                hc.dev<pgorb_kf_pose>(pk.Pose), min_x, max_x, min_y, max_y, hc.dev<int32_t>(pk.S),
                                                                npoints, hc.dev<pgorb_map_point>(pk.P), hc.dev(pk.PD), hc.dev(pk.B), qc,
                                                                hc.dev<int32_t>(oNQ), hc.dev<int32_t>(oQ), (int)th, hc.dev<int32_t>(oA),
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
