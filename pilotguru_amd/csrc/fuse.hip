// fuse.hip -- ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) on gfx950, monocular.
//
// Restates (thirdparty/orb-slam2):
//   ORBmatcher::Fuse                          src/ORBmatcher.cc:827-979
//   KeyFrame::GetFeaturesInArea / IsInImage   src/KeyFrame.cc:672-716
//   MapPoint::Observations / Replace          src/MapPoint.cc:119-130, 196-232
//
// One call decomposes exactly into two passes (the argument is in pgorb.h and DESIGN.md section 4):
//   k_fuse_match     one lane per (problem, query): the skips, the projection, the image, depth and viewing-angle tests,
//                    PredictScale, then the candidates of the search window in the reference's (ix, iy, insertion) order --
//                    at th = 3 the window spans at most 3 x 3 cells -- with the octave and chi-square tests and the first
//                    smallest distance (strict <).  Everything is read from the state on entry.
//   k_fuse_resolve   one workgroup per problem walks the slots' chains: in every round the earliest waiting query of each
//                    slot (atomicMin) is decided against the slot's current occupant and observation union, so the chains
//                    advance in query order, as many rounds as the longest chain.
// Every float operation follows the reference's cv::Mat arithmetic under the readings of DESIGN.md section 4.
#include "kf_window.h"

#define FUSE_T 1024
#define FUSE_MATCHED (-3)                  // k_fuse_match's provisional action of a query with bestDist <= TH_LOW

struct PgFuseBatch {
    PgKfBatch kb;
    const int32_t* kf; const uint64_t* kfId; const int32_t* kfPoint; const int32_t* obsStart; const uint64_t* obsKf;
    int qcap; const int32_t* nq; const int32_t* queries;
    float invS2[PG_MAXL + 1];
};
// per problem scratch: [qcap] best index / distance / provisional action, chain links, two pending lists; [cap] slot state
struct PgFuseScratch {
    int32_t* best; int32_t* dist; int32_t* act; int32_t* link; int32_t* pendA; int32_t* pendB;
    int32_t* occ; int32_t* cnt; int32_t* last; int32_t* head;
};

__device__ __forceinline__ bool fuse_lists(const PgFuseBatch& B, int mp, uint64_t id)
{
    int lo = B.obsStart[mp], hi = B.obsStart[mp + 1];                 // ascending: binary search
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t v = B.obsKf[mid];
        if (v == id) return true;
        if (v < id) lo = mid + 1; else hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_fuse_match(PgFuseBatch B, PgFuseScratch S)
{
    const PgKfBatch& W = B.kb;
    const int p = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const int nq = min(max(B.nq[p], 0), B.qcap);
    if (q >= nq) return;
    const int64_t qi = (int64_t)p * B.qcap + q;
    const int f = B.kf[p];
    int act = PGORB_FUSE_SKIPPED, bestIdx = -1, bestDist = -1;
    const int mp = B.queries[qi];
    KfQuery Q;
    // :850-854: NULL, isBad(), IsInKeyFrame(pKF); then the front part (:856-897)
    if (mp >= 0 && mp < W.npoints && !(W.pbad && W.pbad[mp]) && !fuse_lists(B, mp, B.kfId[f]) && kf_point_query(W, f, mp, Q)) {
        int bd = 256, bi = -1;
        const bool any = kf_scan(W, f, mp, Q,
                                 [&](int, const pgorb_keypoint& kp) {                          // the chi-square test (:941-948)
                                     const float ex = __fsub_rn(Q.u, kp.x), ey = __fsub_rn(Q.v, kp.y);
                                     const float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                                     return (double)__fmul_rn(e2, B.invS2[kp.octave]) > 5.99; },
                                 [&](int idx, int dist) { if (dist < bd) { bd = dist; bi = idx; } });     // :955-959
        if (any) {
            bestIdx = bi; bestDist = bd;
            act = bd <= TH_LOW ? FUSE_MATCHED : PGORB_FUSE_NO_MATCH;
        }
    }
    S.best[qi] = bestIdx; S.dist[qi] = bestDist; S.act[qi] = act;
}

// head[] is changed by atomicMin in L2: read and reset it at device scope, past the CU's vector cache
__device__ __forceinline__ int fuse_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fuse_store(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// point mp's observations include `id`, or the chain's union does (kf id, the original occupant o0, the absorbed queries)
__device__ __forceinline__ bool fuse_in_union(const PgFuseBatch& B, const PgFuseScratch& S, int64_t rowQ, uint64_t kfId, int o0,
                                              int member, uint64_t id)
{
    if (id == kfId) return true;
    if (o0 >= 0 && fuse_lists(B, o0, id)) return true;
    for (int m = member; m >= 0; m = S.link[rowQ + m])
        if (fuse_lists(B, B.queries[rowQ + m], id)) return true;
    return false;
}

__global__ __launch_bounds__(FUSE_T) void k_fuse_resolve(PgFuseBatch B, PgFuseScratch S, int32_t* __restrict__ actOut,
                                                         int32_t* __restrict__ bestOut, int32_t* __restrict__ distOut,
                                                         int32_t* __restrict__ slotsOut, int32_t* __restrict__ nfused)
{
    const PgKfBatch& W = B.kb;
    const int p = blockIdx.x, tid = threadIdx.x, f = B.kf[p], cap = W.cap;
    const int n = min(max(W.n[f], 0), cap), nq = min(max(B.nq[p], 0), B.qcap);
    const int64_t rowQ = (int64_t)p * B.qcap, rowS = (int64_t)p * cap;
    const uint64_t kfId = B.kfId[f];
    __shared__ int sNext, sFused;
    if (tid == 0) { sNext = 0; sFused = 0; }
    for (int s = tid; s < n; s += FUSE_T) {
        int o = B.kfPoint ? B.kfPoint[(int64_t)f * cap + s] : -1;
        if (o >= W.npoints) o = -1;
        S.occ[rowS + s] = o;
        S.cnt[rowS + s] = o >= 0 ? B.obsStart[o + 1] - B.obsStart[o] : 0;
        S.last[rowS + s] = -1;
        fuse_store(&S.head[rowS + s], 0x7FFFFFFF);
    }
    __syncthreads();
    // the matched queries, in any order (the rounds restore query order per slot)
    for (int q = tid; q < nq; q += FUSE_T)
        if (S.act[rowQ + q] == FUSE_MATCHED) S.pendA[rowQ + atomicAdd(&sNext, 1)] = q;
    __syncthreads();
    int npend = sNext;
    int32_t* pend = S.pendA + rowQ;
    int32_t* next = S.pendB + rowQ;
    int fused = 0;
    while (npend > 0) {
        __syncthreads();
        if (tid == 0) sNext = 0;
        for (int i = tid; i < npend; i += FUSE_T) {
            const int q = pend[i];
            atomicMin(&S.head[rowS + S.best[rowQ + q]], q);
        }
        __syncthreads();
        for (int i = tid; i < npend; i += FUSE_T) {
            const int q = pend[i], s = S.best[rowQ + q];
            if (fuse_load(&S.head[rowS + s]) != q) { next[atomicAdd(&sNext, 1)] = q; continue; }
            fuse_store(&S.head[rowS + s], 0x7FFFFFFF);                     // this thread alone owns slot s in this round
            fused++;
            const int o0 = B.kfPoint ? B.kfPoint[(int64_t)f * cap + s] : -1;
            const int o0v = o0 < W.npoints ? o0 : -1;
            const int mp = B.queries[rowQ + q];
            const int nobs = B.obsStart[mp + 1] - B.obsStart[mp];
            int act;
            if (o0v >= 0 && W.pbad && W.pbad[o0v]) {
                act = PGORB_FUSE_KF_POINT_BAD;                                 // :966-967: nothing changes
            } else if (S.occ[rowS + s] < 0) {
                act = PGORB_FUSE_ADDED;                                        // :974-976: AddObservation(pKF) + AddMapPoint
                S.occ[rowS + s] = mp;
                S.cnt[rowS + s] = nobs + 1;
                S.link[rowQ + q] = -1;
                S.last[rowS + s] = q;
            } else {
                const int c = S.cnt[rowS + s];
                int add = 0;                                                   // Replace: the survivor observes the union
                for (int k = B.obsStart[mp], ke = B.obsStart[mp + 1]; k < ke; k++)
                    add += !fuse_in_union(B, S, rowQ, kfId, o0v, S.last[rowS + s], B.obsKf[k]);
                if (c > nobs) act = PGORB_FUSE_MERGED_INTO_KF_POINT;          // pMP->Replace(pMPinKF) (:968-969)
                else { act = PGORB_FUSE_REPLACED_KF_POINT; S.occ[rowS + s] = mp; }   // pMPinKF->Replace(pMP) (:970-971)
                S.cnt[rowS + s] = c + add;
                S.link[rowQ + q] = S.last[rowS + s];
                S.last[rowS + s] = q;
            }
            S.act[rowQ + q] = act;
        }
        __syncthreads();
        npend = sNext;
        int32_t* t = pend; pend = next; next = t;
    }
    atomicAdd(&sFused, fused);
    __syncthreads();
    for (int q = tid; q < nq; q += FUSE_T) {
        actOut[rowQ + q] = S.act[rowQ + q];
        if (bestOut) bestOut[rowQ + q] = S.best[rowQ + q];
        if (distOut) distOut[rowQ + q] = S.dist[rowQ + q];
    }
    if (slotsOut)
        for (int s = tid; s < n; s += FUSE_T) slotsOut[rowS + s] = S.occ[rowS + s];
    if (tid == 0) nfused[p] = sFused;
}

PgKfPack::PgKfPack(PgHostCall& s, const PgKfFrame* f, int nframes, int npoints) : nframes(nframes), cap(1), npoints(npoints)
{
    for (int k = 0; k < nframes; k++) cap = std::max(cap, f[k].n);
    const size_t slots = (size_t)nframes * cap, np = std::max(npoints, 1);
    K = s.region(PG_UP, slots * sizeof(pgorb_keypoint)); D = s.region(PG_UP, slots * 32); S = s.region(PG_UP, slots * 4);
    Pose = s.region(PG_UP, nframes * sizeof(pgorb_kf_pose)); N = s.region(PG_UP, (size_t)nframes * 4); F = s.region(PG_UP, (size_t)nframes * 4);
    P = s.region(PG_UP, np * sizeof(pgorb_map_point)); PD = s.region(PG_UP, np * 32); B = s.region(PG_UP, np);
    GS = GI = 0;
}
void PgKfPack::device(PgHostCall& s)
{
    GS = s.region(PG_DEV, (size_t)nframes * (PGORB_GRID_CELLS + 1) * 4); GI = s.region(PG_DEV, (size_t)nframes * cap * 4);
}
void PgKfPack::pack(PgHostCall& s, const PgKfFrame* f, const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad) const
{
    const size_t kb = sizeof(pgorb_keypoint);
    for (int k = 0; k < nframes; k++) {
        const size_t n = f[k].n, slot = (size_t)k * cap;
        s.host<int32_t>(N)[k] = f[k].n; s.host<int32_t>(F)[k] = k;
        s.put(K, f[k].kps, n * kb, slot * kb, cap * kb);
        s.put(D, f[k].desc, n * 32, slot * 32, (size_t)cap * 32);
        memset(s.host(S) + slot * 4, 0xFF, (size_t)cap * 4);
        s.put(S, f[k].slots, n * 4, slot * 4);
        s.put(Pose, f[k].pose, sizeof(pgorb_kf_pose), k * sizeof(pgorb_kf_pose));
    }
    s.put(P, points, (size_t)npoints * sizeof(pgorb_map_point));
    s.put(PD, point_desc, (size_t)npoints * 32);
    s.put(B, point_bad, npoints, 0, npoints);
}
int PgKfPack::grid(pgorb_ctx* c, PgHostCall& s, float min_x, float max_x, float min_y, float max_y) const
{
    return pgorb_frame_grid_batch_device(c, s.dev<pgorb_keypoint>(K), s.dev<int32_t>(N), nframes, cap, min_x, max_x, min_y, max_y,
                                         s.dev<int32_t>(GS), s.dev<int32_t>(GI), nullptr);
}

extern "C" {

int pgorb_fuse_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                            const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf, int nprob,
                            const uint64_t* d_kf_id, const pgorb_kf_pose* d_pose, float min_x, float max_x, float min_y, float max_y,
                            const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
                            const uint8_t* d_point_bad, const int32_t* d_obs_start, const uint64_t* d_obs_kf,
                            int qcap, const int32_t* d_nq, const int32_t* d_queries, float th,
                            int32_t* d_action, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_kf_point_out, int32_t* d_nfused,
                            void* stream)
{
    PgFuseBatch B = {{d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_pose, npoints, d_points, d_point_desc, d_point_bad},
                     d_kf, d_kf_id, d_kf_point, d_obs_start, d_obs_kf, qcap, d_nq, d_queries};
    int rc;
    if (pg_kf_begin(c, "bad argument to pgorb_fuse_batch_device",
                    qcap >= 1 && (!nprob || (d_kf && d_kf_id && d_nq && d_queries && d_action && d_nfused && d_obs_start)) &&
                        (!npoints || d_obs_kf), B.kb, nprob, min_x, max_x, min_y, max_y, th, rc)) return rc;
    pgorb_scale_tables(c, nullptr, nullptr, nullptr, B.invS2);
    const hipStream_t s = (hipStream_t)stream;
    const size_t rq = (size_t)nprob * qcap * 4, rs = (size_t)nprob * cap * 4;
    PgCarve cv;
    size_t off[10];
    for (int k = 0; k < 10; k++) off[k] = cv.take(k < 6 ? rq : rs);
    void* scr;
    if ((rc = pg_ctx_scratch(c, cv.o, s, &scr))) return rc;
    int32_t* a[10];
    for (int k = 0; k < 10; k++) a[k] = (int32_t*)((uint8_t*)scr + off[k]);
    const PgFuseScratch S = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]};
    hipLaunchKernelGGL(k_fuse_match, dim3((unsigned)((qcap + 255) / 256), (unsigned)nprob), dim3(256), 0, s, B, S);
    hipLaunchKernelGGL(k_fuse_resolve, dim3((unsigned)nprob), dim3(FUSE_T), 0, s, B, S, d_action, d_best_idx, d_best_dist,
                       d_kf_point_out, d_nfused);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_fuse_match / k_fuse_resolve launch failed");
    return pg_ctx_scratch_done(c, s);
}

// one key frame through host buffers: a one-problem batch; the inputs are checked here
int pgorb_fuse(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* pose, uint64_t kf_id,
               float min_x, float max_x, float min_y, float max_y, const int32_t* kf_point, int npoints, const pgorb_map_point* points,
               const uint8_t* point_desc, const uint8_t* point_bad, const int32_t* obs_start, const uint64_t* obs_kf, int nq,
               const int32_t* queries, float th, int32_t* action, int32_t* best_idx, int32_t* best_dist, int32_t* kf_point_out)
{
    if (!c) return PGORB_E_ARG;
    const char* bad = "bad argument to pgorb_fuse";
    if (n < 0 || npoints < 0 || nq < 0 || !pose || !obs_start || !(max_x > min_x) || !(max_y > min_y) || !(th > 0.0f) ||
        (n && (!kps || !desc)) || (npoints && (!points || !point_desc)) || (nq && (!queries || !action)))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (n > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (obs_start[0] != 0) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: obs_start[0] must be 0");
    for (int i = 0; i < npoints; i++) {
        if (obs_start[i + 1] < obs_start[i]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: obs_start decreases");
        for (int k = obs_start[i] + 1; k < obs_start[i + 1]; k++)
            if (!(obs_kf[k - 1] < obs_kf[k])) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: an observation list is unsorted or repeats a key frame");
    }
    const int nobs = obs_start[npoints];
    if (nobs && !obs_kf) return pg_ctx_fail(c, PGORB_E_ARG, bad);
    auto lists = [&](int mp, uint64_t id) {
        for (int k = obs_start[mp]; k < obs_start[mp + 1]; k++) if (obs_kf[k] == id) return true;
        return false;
    };
    std::vector<uint8_t> seen((size_t)npoints, 0);
    for (int i = 0; kf_point && i < n; i++) {
        const int o = kf_point[i];
        if (o < -1 || o >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: a slot's point index is out of range");
        if (o < 0 || (point_bad && point_bad[o])) continue;              // a bad occupant only makes its queries KF_POINT_BAD
        if (seen[o]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: a point holds two slots of the key frame");
        seen[o] = 1;
        if (!lists(o, kf_id)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: a slot's point does not list the key frame");
    }
    std::fill(seen.begin(), seen.end(), 0);
    for (int q = 0; q < nq; q++) {
        const int m = queries[q];
        if (m < -1 || m >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: a query index is out of range");
        if (m < 0) continue;
        if (seen[m]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_fuse: a map point is queried twice");
        seen[m] = 1;
    }
    if (kf_point_out) for (int i = 0; i < n; i++) kf_point_out[i] = kf_point ? kf_point[i] : -1;
    if (!nq) return 0;
    for (int q = 0; q < nq; q++) { action[q] = PGORB_FUSE_SKIPPED; if (best_idx) best_idx[q] = -1; if (best_dist) best_dist[q] = -1; }
    const PgKfFrame f = {kps, desc, kf_point, pose, n};
    PgHostCall hc(c);
    PgKfPack pk(hc, &f, 1, npoints);
    const int cap = pk.cap;
    const size_t oId = hc.region(PG_UP, 8), oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4),
                 oOK = hc.region(PG_UP, (size_t)std::max(nobs, 1) * 8), oNQ = hc.region(PG_UP, 4), oQ = hc.region(PG_UP, (size_t)nq * 4),
                 oA = hc.region(PG_DOWN, (size_t)nq * 4), oBI = hc.region(PG_DOWN, (size_t)nq * 4), oBD = hc.region(PG_DOWN, (size_t)nq * 4),
                 oSO = hc.region(PG_DOWN, (size_t)cap * 4), oNF = hc.region(PG_DOWN, 4);
    pk.device(hc);
    int rc = hc.begin();
    if (rc) return rc;
    pk.pack(hc, &f, points, point_desc, point_bad);
    hc.put(oId, &kf_id, 8);
    hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4);
    hc.put(oOK, obs_kf, (size_t)nobs * 8);
    hc.put(oNQ, &nq, 4);
    hc.put(oQ, queries, (size_t)nq * 4);
    if ((rc = hc.run([&] {
            const int r = pk.grid(c, hc, min_x, max_x, min_y, max_y);
            return r ? r : pgorb_fuse_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), cap, hc.dev<int32_t>(pk.GS),
                                                   hc.dev<int32_t>(pk.GI), hc.dev<int32_t>(pk.F), 1, hc.dev<uint64_t>(oId), hc.dev<pgorb_kf_pose>(pk.Pose),
                                                   min_x, max_x, min_y, max_y, hc.dev<int32_t>(pk.S), npoints, hc.dev<pgorb_map_point>(pk.P),
                                                   hc.dev(pk.PD), hc.dev(pk.B), hc.dev<int32_t>(oOS), hc.dev<uint64_t>(oOK), nq,
                                                   hc.dev<int32_t>(oNQ), hc.dev<int32_t>(oQ), th, hc.dev<int32_t>(oA), hc.dev<int32_t>(oBI),
                                                   hc.dev<int32_t>(oBD), hc.dev<int32_t>(oSO), hc.dev<int32_t>(oNF), nullptr); }))) return rc;
    memcpy(action, hc.host(oA), (size_t)nq * 4);
    if (best_idx) memcpy(best_idx, hc.host(oBI), (size_t)nq * 4);
    if (best_dist) memcpy(best_dist, hc.host(oBD), (size_t)nq * 4);
    if (kf_point_out) memcpy(kf_point_out, hc.host(oSO), (size_t)n * 4);
    return *hc.host<int32_t>(oNF);
}

}  // extern "C"
