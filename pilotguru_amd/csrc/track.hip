// track.hip -- the tracking thread's three projection matchers on gfx950 with the projection on the device: poses, a resident
// map-point table and indices go in, matches come out.
//
// Restates (thirdparty/orb-slam2):
//   Tracking::SearchLocalPoints               src/Tracking.cc:1134-1184
//   Frame::isInFrustum                        src/Frame.cc:273-329
//   ORBmatcher::SearchByProjection            src/ORBmatcher.cc:1342-1385 (last frame, the front part), :1480-1532 (key frame, the front part)
//   MapPoint::GetMin/MaxDistanceInvariance    src/MapPoint.cc:390-400
//
// Every call is a front part and the two passes of window_match.hip (proj_match.h):
//   k_track_slots   (SearchLocalPoints only) one lane per (pair, keypoint): the first loop (:1137-1153) -- a slot holding a bad
//                   point is cleared, any other slot marks its point as seen (one bit per table point and pair) and gives the
//                   keypoint its "holds a point with observations" flag.
//   k_track_front   one lane per (pair, query): the skips, Rcw*P + tcw, the projection, the Frame's inclusive bounds and, by
//                   form, the distance / viewing-angle tests and PredictScale; it writes the query arrays k_proj_candidates and
//                   k_search_by_projection read (valid, x, y, level, aux, the gathered descriptor, ...), which then decide as
//                   they do for a caller who passes those arrays.
// Every float operation follows the reference's cv::Mat arithmetic under the readings of DESIGN.md section 4.
#include "kf_window.h"
#include "proj_match.h"
#include <string>

#define TRACK_LOCAL 0            // the modes of the two passes: local map points, last frame, key frame
#define TRACK_LAST 1
#define TRACK_KF 2
#define TRACK_MAX_POINTS (1 << 20)   // SearchLocalPoints: table points (their seen marks are 128 KiB a pair)

struct PgTrackBatch {
    // (b), (c): the last frame / the key frame of pair p is frame pairOther[p] of otherK (keypoints otherCap apart, counts otherN)
    const pgorb_keypoint* otherK; const int32_t* otherN; int otherCap; const int32_t* pairOther;
    const pgorb_kf_pose* pose;             // [npairs]
    int npoints; const pgorb_map_point* pts; const uint8_t* pdesc; const uint8_t* pbad; const uint8_t* pobs;
    int qcap; const int32_t* nq;           // (a) [npairs]; (b), (c): the other frame's keypoint count
    const int32_t* queries;                // [npairs][qcap] table indices: the queries / last_point / kf_point
    const uint8_t* qflag;                  // [npairs][qcap] or null: query_seen / last_outlier / already_found
    const uint32_t* seen; int seenWords;   // (a) [npairs][seenWords] or null
    float minX, maxX, minY, maxY, cosLimit, logSf; int nlevels;
    // what the two passes read, [npairs][qcap]
    uint8_t* valid; float* x; float* y; int32_t* level; float* aux; uint8_t* desc; uint8_t* hasObs;
    uint8_t* found; float* dist3d; float* minDist; float* maxDist; int32_t* nqOut;
    // the caller's outputs, [npairs][qcap] (any may be null): in_view / valid, the projection, level, view_cos / dist3d
    uint8_t* oValid; float* oX; float* oY; int32_t* oLevel; float* oAux;
    int32_t* nToMatch;                     // (a) [npairs], zeroed before the launch
};

// (a) the first loop of SearchLocalPoints over the frame's slots
__global__ __launch_bounds__(256) void k_track_slots(const int32_t* __restrict__ n, int cap, const int32_t* __restrict__ pairFrame,
                                                     const int32_t* __restrict__ kpPoint, int npoints, const uint8_t* __restrict__ pbad,
                                                     const uint8_t* __restrict__ pobs, uint32_t* __restrict__ seen, int seenWords,
                                                     uint8_t* __restrict__ has, int32_t* __restrict__ kpOut)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const int f = pairFrame ? pairFrame[p] : p;
    const int64_t ki = (int64_t)p * cap + i;
    int s = i < min(max(n[f], 0), cap) ? kpPoint[ki] : -1;
    if (s < 0 || s >= npoints) s = -1;
    if (s >= 0) {
        if (pbad && pbad[s]) s = -1;                                                    // :1142-1145
        else atomicOr(&seen[(int64_t)p * seenWords + (s >> 5)], 1u << (s & 31));         // mnLastFrameSeen = mCurrentFrame.mnId (:1149)
    }
    has[ki] = s >= 0 ? (pobs ? (pobs[s] != 0) : 1) : 0;                                  // ORBmatcher.cc:79-81
    if (kpOut) kpOut[ki] = s;
}

// the Frame's float bounds, inclusive on both sides (Frame.cc:295-298, ORBmatcher.cc:1377-1380, :1511-1514); a NaN is outside
__device__ __forceinline__ bool track_in_bounds(const PgTrackBatch& B, float u, float v)
{
    return (u >= B.minX) & (u <= B.maxX) & (v >= B.minY) & (v <= B.maxY);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_track_front(PgTrackBatch B)
{
    const int p = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const int other = MODE == TRACK_LOCAL ? 0 : B.pairOther[p];
    const int nq = MODE == TRACK_LOCAL ? min(max(B.nq[p], 0), B.qcap) : min(min(max(B.otherN[other], 0), B.otherCap), B.qcap);
    if (MODE != TRACK_LOCAL && q == 0) B.nqOut[p] = nq;
    if (q >= nq) return;
    const int64_t qi = (int64_t)p * B.qcap + q;
    int mp = B.queries[qi];
    if (mp < 0 || mp >= B.npoints) mp = -1;                                             // NULL
    bool ok = mp >= 0 && !(B.qflag && B.qflag[qi]);             // query_seen (Tracking.cc:1161) / mvbOutlier (:1361) / sAlreadyFound (:1498)
    if (MODE == TRACK_LOCAL) ok = ok && !(B.seen && ((B.seen[(int64_t)p * B.seenWords + (mp >> 5)] >> (mp & 31)) & 1u));
    if (MODE != TRACK_LAST) ok = ok && !(B.pbad && B.pbad[mp]);                          // (the last-frame form has no isBad() test)
    float u = 0.0f, v = 0.0f, d3 = 0.0f, viewCos = 0.0f;
    int lvl = 0;
    if (ok) {
        const pgorb_map_point P = B.pts[mp];
        const pgorb_kf_pose& C = B.pose[p];
        float pc[3];
        kf_to_camera(C, P.pos, pc);
        if (MODE == TRACK_LOCAL) ok = !(pc[2] < 0.0f);                                  // Frame.cc:287
        const float invz = __fdiv_rn(1.0f, pc[2]);
        if (MODE == TRACK_LAST) ok = !(invz < 0.0f);                                    // ORBmatcher.cc:1371
        u = __fadd_rn(__fmul_rn(__fmul_rn(C.fx, pc[0]), invz), C.cx);                   // fx*xc*invzc + cx, in the written order
        v = __fadd_rn(__fmul_rn(__fmul_rn(C.fy, pc[1]), invz), C.cy);
        ok = ok && track_in_bounds(B, u, v);
        if (MODE != TRACK_LAST && ok) {
            const float po0 = __fsub_rn(P.pos[0], C.Ow[0]), po1 = __fsub_rn(P.pos[1], C.Ow[1]), po2 = __fsub_rn(P.pos[2], C.Ow[2]);
            d3 = cnm_f(cnm_normd(po0, po1, po2));
            if (MODE == TRACK_LOCAL) {
                ok = kf_depth_ok(P, d3);                                                // Frame.cc:301-307
                if (ok) {
                    viewCos = cnm_f(__ddiv_rn(cnm_dotd(po0, po1, po2, P.normal[0], P.normal[1], P.normal[2]), (double)d3));
                    ok = !(viewCos < B.cosLimit);                                       // :312-315
                }
                if (ok) lvl = pg_predict_scale(P.max_distance, d3, B.logSf, B.nlevels);  // :318
            }
        }
        if (ok) {
            B.x[qi] = u; B.y[qi] = v;
            const uint4* src = reinterpret_cast<const uint4*>(B.pdesc + (int64_t)mp * 32);
            uint4* dst = reinterpret_cast<uint4*>(B.desc + qi * 32);
            dst[0] = src[0]; dst[1] = src[1];
            if (MODE == TRACK_LOCAL) { B.level[qi] = lvl; B.aux[qi] = viewCos; }
            else {
                const pgorb_keypoint kp = B.otherK[(int64_t)other * B.otherCap + q];
                B.aux[qi] = kp.angle;                                                    // mvKeysUn[i].angle (:1428, :1561)
                if (MODE == TRACK_LAST) B.level[qi] = kp.octave;                         // mvKeys[i].octave (:1382)
            }
            if (MODE == TRACK_KF) { B.found[qi] = 0; B.dist3d[qi] = d3; B.minDist[qi] = P.min_distance; B.maxDist[qi] = P.max_distance; }
            else B.hasObs[qi] = B.pobs ? (B.pobs[mp] != 0) : 1;
        }
    }
    B.valid[qi] = ok;
    if (B.oValid) B.oValid[qi] = ok;
    if (B.oX) B.oX[qi] = ok ? u : 0.0f;
    if (B.oY) B.oY[qi] = ok ? v : 0.0f;
    if (B.oLevel) B.oLevel[qi] = ok ? lvl : 0;
    if (B.oAux) B.oAux[qi] = ok ? (MODE == TRACK_LOCAL ? viewCos : d3) : 0.0f;
    if (MODE == TRACK_LOCAL) {
        const unsigned long long m = __ballot(ok);
        if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&B.nToMatch[p], __popcll(m));   // nToMatch (:1169)
    }
}

// what a form passes beyond the frames, the pose and the table
struct PgTrackCall {
    int mode;
    const pgorb_keypoint* otherK; const int32_t* otherN; int otherCap; const int32_t* pairOther; const int32_t* kpPoint; const uint8_t* kpHasPoint;
    int qcap; const int32_t* nq; const int32_t* queries; const uint8_t* qflag;
    float cosLimit, th, nnratio; int orbDist, checkOrientation;
    uint8_t* oValid; float* oX; float* oY; int32_t* oLevel; float* oAux; int32_t* kpOut; int32_t* nToMatch;
};

static int pg_track_batch(pgorb_ctx* c, const char* bad, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                          const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs, float min_x,
                          float max_x, float min_y, float max_y, const pgorb_kf_pose* d_pose, int npoints, const pgorb_map_point* d_points,
                          const uint8_t* d_point_desc, const uint8_t* d_point_bad, const uint8_t* d_point_has_obs, const PgTrackCall& t,
                          int32_t* d_assigned, int32_t* d_nmatches, hipStream_t stream)
{
    if (!c) return PGORB_E_ARG;
    const int mode = t.mode, qcap = t.qcap;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || npairs < 0 || qcap < 0 || npoints < 0 ||
        (npairs && (!d_pose || !d_assigned || !d_nmatches)) || (npoints && (!d_points || !d_point_desc)) ||
        (npairs && qcap && !t.queries) || (npairs && mode == TRACK_LOCAL && (!t.nq || !t.oValid || !t.nToMatch)) ||
        (npairs && mode != TRACK_LOCAL && (!t.pairOther || !t.otherK || !t.otherN)) || !(max_x > min_x) || !(max_y > min_y) || !(t.th > 0.0f))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (cap > LIST_MAX_N || qcap > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
    if (mode == TRACK_LOCAL && npoints > TRACK_MAX_POINTS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_search_local_points: more than 1048576 table points (the seen marks of a pair)");
    if (!npairs) return 0;
    if (!(pgorb_levels(c) > 0) || !(pgorb_log_scale_factor(c) > 0.0f)) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    const size_t rows = (size_t)npairs * std::max(qcap, 1), slots = (size_t)npairs * cap;
    const bool marks = mode == TRACK_LOCAL && t.kpPoint;
    const int seenWords = marks ? (std::max(npoints, 1) + 31) / 32 : 0;
    PgCarve cv;
    const size_t oV = cv.take(rows), oX = cv.take(rows * 4), oY = cv.take(rows * 4), oL = cv.take(rows * 4), oA = cv.take(rows * 4),
                 oD = cv.take(rows * 32), oO = cv.take(rows), oF = cv.take(mode == TRACK_KF ? rows : 0),
                 oD3 = cv.take(mode == TRACK_KF ? rows * 4 : 0), oMin = cv.take(mode == TRACK_KF ? rows * 4 : 0),
                 oMax = cv.take(mode == TRACK_KF ? rows * 4 : 0), oNq = cv.take((size_t)npairs * 4), oHas = cv.take(marks ? slots : 0),
                 oSeen = cv.take((size_t)npairs * seenWords * 4);
    PgLists Ls;
    void* extra;
    int rc = pg_proj_begin(c, cap, qcap, npairs, cv.o, stream, &Ls, &extra);
    if (rc) return rc;
    uint8_t* e = (uint8_t*)extra;
    PgTrackBatch T;
    T.otherK = t.otherK; T.otherN = t.otherN; T.otherCap = t.otherCap; T.pairOther = t.pairOther; T.pose = d_pose;
    T.npoints = npoints; T.pts = d_points; T.pdesc = d_point_desc; T.pbad = d_point_bad; T.pobs = d_point_has_obs;
    T.qcap = qcap; T.nq = t.nq; T.queries = t.queries; T.qflag = t.qflag;
    T.seen = marks ? (const uint32_t*)(e + oSeen) : nullptr; T.seenWords = seenWords;
    T.minX = min_x; T.maxX = max_x; T.minY = min_y; T.maxY = max_y; T.cosLimit = t.cosLimit;
    T.logSf = pgorb_log_scale_factor(c); T.nlevels = pgorb_levels(c);
    T.valid = e + oV; T.x = (float*)(e + oX); T.y = (float*)(e + oY); T.level = (int32_t*)(e + oL); T.aux = (float*)(e + oA);
    T.desc = e + oD; T.hasObs = e + oO; T.found = e + oF; T.dist3d = (float*)(e + oD3); T.minDist = (float*)(e + oMin);
    T.maxDist = (float*)(e + oMax); T.nqOut = (int32_t*)(e + oNq);
    T.oValid = t.oValid; T.oX = t.oX; T.oY = t.oY; T.oLevel = t.oLevel; T.oAux = t.oAux; T.nToMatch = t.nToMatch;
    const uint8_t* has = t.kpHasPoint;
    if (mode == TRACK_LOCAL) {
        if (hipMemsetAsync(t.nToMatch, 0, (size_t)npairs * 4, stream) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
        if (marks) {
            if (hipMemsetAsync(e + oSeen, 0, (size_t)npairs * seenWords * 4, stream) != hipSuccess)
                return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
            hipLaunchKernelGGL(k_track_slots, dim3((unsigned)((cap + 255) / 256), (unsigned)npairs), dim3(256), 0, stream, d_n, cap, d_pair_frame,
                               t.kpPoint, npoints, d_point_bad, d_point_has_obs, (uint32_t*)(e + oSeen), seenWords, e + oHas, t.kpOut);
            has = e + oHas;
        } else if (t.kpOut && hipMemsetAsync(t.kpOut, 0xFF, slots * 4, stream) != hipSuccess)
            return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    }
    if (qcap) {
        const dim3 grid((unsigned)((qcap + 255) / 256), (unsigned)npairs);
        if (mode == TRACK_LOCAL) hipLaunchKernelGGL(k_track_front<TRACK_LOCAL>, grid, dim3(256), 0, stream, T);
        else if (mode == TRACK_LAST) hipLaunchKernelGGL(k_track_front<TRACK_LAST>, grid, dim3(256), 0, stream, T);
        else hipLaunchKernelGGL(k_track_front<TRACK_KF>, grid, dim3(256), 0, stream, T);
    } else if (mode != TRACK_LOCAL && hipMemsetAsync(T.nqOut, 0, (size_t)npairs * 4, stream) != hipSuccess)
        return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_track_front launch failed");
    PgProjBatch B;
    B.K = d_kps; B.D = d_desc; B.n = d_n; B.cap = cap; B.gstart = d_grid_start; B.gidx = d_grid_idx; B.pairFrame = d_pair_frame;
    B.kpHasPoint = has; B.qcap = qcap; B.nq = mode == TRACK_LOCAL ? t.nq : T.nqOut; B.valid = T.valid; B.x = T.x; B.y = T.y;
    B.level = T.level; B.aux = T.aux; B.desc = T.desc; B.hasObs = T.hasObs; B.th = t.th;
    B.found = T.found; B.dist3d = T.dist3d; B.minDist = T.minDist; B.maxDist = T.maxDist; B.logSf = T.logSf;
    B.orbDist = mode == TRACK_KF ? t.orbDist : TH_HIGH;
    return pg_proj_run(c, B, npairs, min_x, max_x, min_y, max_y, mode, t.nnratio, t.checkOrientation, Ls, d_assigned, d_nmatches, stream);
}

// ---- the single calls: one pair through host buffers -------------------------------------------------------------------------------
// what the three single calls check alike, on the host and before anything is staged: counts, pointers, bounds, th, and every table
// index inside [lo, npoints)
static const char* pg_track_args(int n, const void* kps, const void* desc, const void* pose, float min_x, float max_x, float min_y,
                                 float max_y, float th, int npoints, const void* points, const void* point_desc, int nq, const int32_t* queries,
                                 int lo, const void* assigned)
{
    if (n < 0 || nq < 0 || npoints < 0 || !pose || (n && (!kps || !desc || !assigned)) || (npoints && (!points || !point_desc)) ||
        (nq && !queries)) return "a count is negative or a pointer is NULL";
    if (!(max_x > min_x) || !(max_y > min_y)) return "the bounds are empty";
    if (!(th > 0.0f)) return "th must be positive";
    for (int q = 0; q < nq; q++)
        if (queries[q] < lo || queries[q] >= npoints) return "a table index is out of range";
    return nullptr;
}

struct PgTrackHost {
    const pgorb_keypoint* kps; const uint8_t* desc; int n;                  // the current frame
    const pgorb_keypoint* okps; int nother;                                 // the last frame / the key frame (forms b, c)
    const pgorb_kf_pose* pose; const int32_t* kpPoint; const uint8_t* kpHasPoint;
    int npoints; const pgorb_map_point* points; const uint8_t* pdesc; const uint8_t* pbad; const uint8_t* pobs;
    int nq; const int32_t* queries; const uint8_t* qflag;
};

static int pg_track_host(pgorb_ctx* c, const char* bad, int mode, const PgTrackHost& h, float min_x, float max_x, float min_y, float max_y,
                         float cosLimit, float th, float nnratio, int orbDist, int checkOrientation, uint8_t* rValid, float* rX, float* rY,
                         int32_t* rLevel, float* rAux, int32_t* kpOut, int32_t* nToMatch, int32_t* assigned)
{
    const int n = h.n, nq = h.nq, npoints = h.npoints;
    for (int i = 0; i < n; i++) assigned[i] = -1;
    for (int q = 0; q < nq; q++) {
        if (rValid) rValid[q] = 0;
        if (rX) rX[q] = 0.0f;
        if (rY) rY[q] = 0.0f;
        if (rLevel) rLevel[q] = 0;
        if (rAux) rAux[q] = 0.0f;
    }
    if (nToMatch) *nToMatch = 0;
    if (kpOut) for (int i = 0; i < n; i++) kpOut[i] = h.kpPoint ? ((h.pbad && h.kpPoint[i] >= 0 && h.pbad[h.kpPoint[i]]) ? -1 : h.kpPoint[i]) : -1;
    if (!nq) return 0;
    const int cap = std::max(n, 1), ocap = std::max(h.nother, 1), np = std::max(npoints, 1);
    if (n > LIST_MAX_N || nq > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
    if (pg_sbp_lds(n, nq) > PG_SBP_LDS_MAX) return pg_ctx_fail(c, PGORB_E_LIMIT, PG_SBP_LDS_MSG);      // (before anything is staged)
    if (mode == TRACK_LOCAL && npoints > TRACK_MAX_POINTS)
        return pg_ctx_fail(c, PGORB_E_LIMIT, "pgorb_search_local_points: more than 1048576 table points (the seen marks of a pair)");
    const size_t kb = sizeof(pgorb_keypoint), q4 = (size_t)nq * 4;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)cap * kb), oK2 = s.region(PG_UP, mode == TRACK_LOCAL ? 0 : (size_t)ocap * kb),
                 oD = s.region(PG_UP, (size_t)cap * 32),
                 oPose = s.region(PG_UP, sizeof(pgorb_kf_pose)), oKP = s.region(PG_UP, h.kpPoint ? (size_t)cap * 4 : 0),
                 oH = s.region(PG_UP, h.kpHasPoint ? cap : 0), oP = s.region(PG_UP, np * sizeof(pgorb_map_point)), oPD = s.region(PG_UP, (size_t)np * 32),
                 oB = s.region(PG_UP, h.pbad ? np : 0), oO = s.region(PG_UP, h.pobs ? np : 0), oQ = s.region(PG_UP, q4),
                 oQF = s.region(PG_UP, h.qflag ? nq : 0), oAs = s.region(PG_DOWN, (size_t)cap * 4), oR = s.region(PG_DOWN, 8),
                 oV = s.region(PG_DOWN, nq), oX = s.region(PG_DOWN, q4), oY = s.region(PG_DOWN, q4), oL = s.region(PG_DOWN, q4),
                 oA = s.region(PG_DOWN, q4), oKO = s.region(PG_DOWN, (size_t)cap * 4),
                 oGS = s.region(PG_DEV, (size_t)(GRID_CELLS + 1) * 4), oGI = s.region(PG_DEV, (size_t)cap * 4);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t cnt[4] = {n, h.nother, nq, 0};                 // n, the other frame's n, nq, the other frame's number
    s.put(oN, cnt, 16);
    s.put(oK, h.kps, n * kb, 0, cap * kb);
    if (mode != TRACK_LOCAL) s.put(oK2, h.okps, h.nother * kb, 0, ocap * kb);
    s.put(oD, h.desc, (size_t)n * 32); s.put(oPose, h.pose, sizeof(pgorb_kf_pose));
    if (h.kpPoint) { memset(s.host(oKP), 0xFF, (size_t)cap * 4); s.put(oKP, h.kpPoint, (size_t)n * 4); }
    if (h.kpHasPoint) s.put(oH, h.kpHasPoint, n, 0, cap);
    s.put(oP, h.points, (size_t)npoints * sizeof(pgorb_map_point)); s.put(oPD, h.pdesc, (size_t)npoints * 32);
    if (h.pbad) s.put(oB, h.pbad, npoints);
    if (h.pobs) s.put(oO, h.pobs, npoints);
    s.put(oQ, h.queries, q4);
    if (h.qflag) s.put(oQF, h.qflag, nq);
    const PgTrackCall t = {mode, s.dev<pgorb_keypoint>(oK2), s.dev<int32_t>(oN) + 1, ocap, s.dev<int32_t>(oN) + 3, h.kpPoint ? s.dev<int32_t>(oKP) : nullptr, h.kpHasPoint ? s.dev(oH) : nullptr,
                           nq, s.dev<int32_t>(oN) + 2, s.dev<int32_t>(oQ), h.qflag ? s.dev(oQF) : nullptr, cosLimit, th, nnratio, orbDist,
                           checkOrientation, s.dev(oV), s.dev<float>(oX), s.dev<float>(oY), s.dev<int32_t>(oL), s.dev<float>(oA),
                           s.dev<int32_t>(oKO), s.dev<int32_t>(oR) + 1};
    if ((rc = s.run([&] {
            const int r = pgorb_frame_grid_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), 1, cap, min_x, max_x, min_y, max_y,
                                                        s.dev<int32_t>(oGS), s.dev<int32_t>(oGI), nullptr);
            return r ? r : pg_track_batch(c, bad, s.dev<pgorb_keypoint>(oK), s.dev(oD), s.dev<int32_t>(oN), cap, s.dev<int32_t>(oGS),
                                          s.dev<int32_t>(oGI), nullptr, 1, min_x, max_x, min_y, max_y, s.dev<pgorb_kf_pose>(oPose), npoints,
                                          s.dev<pgorb_map_point>(oP), s.dev(oPD), h.pbad ? s.dev(oB) : nullptr, h.pobs ? s.dev(oO) : nullptr, t,
                                          s.dev<int32_t>(oAs), s.dev<int32_t>(oR), nullptr); }))) return rc;
    memcpy(assigned, s.host(oAs), (size_t)n * 4);
    if (rValid) memcpy(rValid, s.host(oV), nq);
    if (rX) memcpy(rX, s.host(oX), q4);
    if (rY) memcpy(rY, s.host(oY), q4);
    if (rLevel) memcpy(rLevel, s.host(oL), q4);
    if (rAux) memcpy(rAux, s.host(oA), q4);
    if (kpOut) memcpy(kpOut, s.host(oKO), (size_t)n * 4);
    if (nToMatch) *nToMatch = s.host<int32_t>(oR)[1];
    return s.host<int32_t>(oR)[0];
}

extern "C" {

int pgorb_search_local_points(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x, float min_y,
                              float max_y, const pgorb_kf_pose* pose, const int32_t* kp_point, int npoints, const pgorb_map_point* points,
                              const uint8_t* point_desc, const uint8_t* point_bad, const uint8_t* point_has_obs, int nq,
                              const int32_t* queries, const uint8_t* query_seen, float viewing_cos_limit, float th, float nnratio,
                              uint8_t* in_view, float* proj_x, float* proj_y, int32_t* level, float* view_cos, int32_t* kp_point_out,
                              int32_t* n_to_match, int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    const char* why = pg_track_args(n, kps, desc, pose, min_x, max_x, min_y, max_y, th, npoints, points, point_desc, nq, queries, 0, assigned);
    if (!why && nq && !in_view) why = "in_view is NULL";
    for (int i = 0; !why && kp_point && i < n; i++)
        if (kp_point[i] < -1 || kp_point[i] >= npoints) why = "a slot's point index is out of range";
    if (!why && nq) {
        std::vector<uint8_t> listed((size_t)npoints, 0);
        for (int q = 0; q < nq && !why; q++) {
            if (listed[queries[q]]) why = "a map point is queried twice";
            listed[queries[q]] = 1;
        }
    }
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_search_local_points: ") + why).c_str());
    const PgTrackHost h = {kps, desc, n, nullptr, 0, pose, kp_point, nullptr, npoints, points, point_desc, point_bad, point_has_obs,
                           nq, queries, query_seen};
    return pg_track_host(c, "bad argument to pgorb_search_local_points", TRACK_LOCAL, h, min_x, max_x, min_y, max_y, viewing_cos_limit, th,
                         nnratio, 0, 0, in_view, proj_x, proj_y, level, view_cos, kp_point_out, n_to_match, assigned);
}

int pgorb_search_local_points_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs, float min_x,
        float max_x, float min_y, float max_y, const pgorb_kf_pose* d_pose, const int32_t* d_kp_point, int npoints,
        const pgorb_map_point* d_points, const uint8_t* d_point_desc, const uint8_t* d_point_bad, const uint8_t* d_point_has_obs, int qcap,
        const int32_t* d_nq, const int32_t* d_queries, const uint8_t* d_query_seen, float viewing_cos_limit, float th, float nnratio,
        uint8_t* d_in_view, float* d_proj_x, float* d_proj_y, int32_t* d_level, float* d_view_cos, int32_t* d_kp_point_out,
        int32_t* d_n_to_match, int32_t* d_assigned, int32_t* d_nmatches, void* stream)
{
    const PgTrackCall t = {TRACK_LOCAL, nullptr, nullptr, 0, nullptr, d_kp_point, nullptr, qcap, d_nq, d_queries, d_query_seen, viewing_cos_limit, th, nnratio, 0, 0,
                           d_in_view, d_proj_x, d_proj_y, d_level, d_view_cos, d_kp_point_out, d_n_to_match};
    return pg_track_batch(c, "bad argument to pgorb_search_local_points_batch_device", d_kps, d_desc, d_n, cap_per_frame, d_grid_start,
                          d_grid_idx, d_pair_frame, npairs, min_x, max_x, min_y, max_y, d_pose, npoints, d_points, d_point_desc, d_point_bad,
                          d_point_has_obs, t, d_assigned, d_nmatches, (hipStream_t)stream);
}

int pgorb_search_by_projection_last_frame(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x,
                                          float min_y, float max_y, const pgorb_kf_pose* pose, const uint8_t* kp_has_point,
                                          const pgorb_keypoint* last_kps, int nlast, const int32_t* last_point, const uint8_t* last_outlier,
                                          int npoints, const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_has_obs,
                                          float th, int check_orientation, uint8_t* valid, float* u, float* v, int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    const char* why = pg_track_args(n, kps, desc, pose, min_x, max_x, min_y, max_y, th, npoints, points, point_desc, nlast, last_point, -1, assigned);
    if (!why && nlast && !last_kps) why = "the last frame's keypoints are NULL";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_search_by_projection_last_frame: ") + why).c_str());
    const PgTrackHost h = {kps, desc, n, last_kps, nlast, pose, nullptr, kp_has_point, npoints, points, point_desc, nullptr, point_has_obs,
                           nlast, last_point, last_outlier};
    return pg_track_host(c, "bad argument to pgorb_search_by_projection_last_frame", TRACK_LAST, h, min_x, max_x, min_y, max_y, 0.0f, th, 0.0f,
                         0, check_orientation, valid, u, v, nullptr, nullptr, nullptr, nullptr, assigned);
}

int pgorb_search_by_projection_last_frame_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, const int32_t* d_pair_last,
        int npairs, float min_x, float max_x, float min_y, float max_y, const pgorb_kf_pose* d_pose, const uint8_t* d_kp_has_point,
        const int32_t* d_last_point, const uint8_t* d_last_outlier, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
        const uint8_t* d_point_has_obs, float th, int check_orientation, uint8_t* d_valid, float* d_u, float* d_v, int32_t* d_assigned,
        int32_t* d_nmatches, void* stream)
{
    const PgTrackCall t = {TRACK_LAST, d_kps, d_n, cap_per_frame, d_pair_last, nullptr, d_kp_has_point, cap_per_frame, nullptr, d_last_point, d_last_outlier, 0.0f, th, 0.0f,
                           0, check_orientation, d_valid, d_u, d_v, nullptr, nullptr, nullptr, nullptr};
    return pg_track_batch(c, "bad argument to pgorb_search_by_projection_last_frame_batch_device", d_kps, d_desc, d_n, cap_per_frame,
                          d_grid_start, d_grid_idx, d_pair_frame, npairs, min_x, max_x, min_y, max_y, d_pose, npoints, d_points, d_point_desc,
                          nullptr, d_point_has_obs, t, d_assigned, d_nmatches, (hipStream_t)stream);
}

int pgorb_search_by_projection_keyframe_pose(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x,
                                             float min_y, float max_y, const pgorb_kf_pose* pose, const uint8_t* kp_has_point,
                                             const pgorb_keypoint* kf_kps, int nkf, const int32_t* kf_point, const uint8_t* already_found,
                                             int npoints, const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad,
                                             float th, int orb_dist, int check_orientation, float* u, float* v, float* dist3d,
                                             int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    const char* why = pg_track_args(n, kps, desc, pose, min_x, max_x, min_y, max_y, th, npoints, points, point_desc, nkf, kf_point, -1, assigned);
    if (!why && nkf && !kf_kps) why = "the key frame's keypoints are NULL";
    if (why) return pg_ctx_fail(c, PGORB_E_ARG, (std::string("pgorb_search_by_projection_keyframe_pose: ") + why).c_str());
    const PgTrackHost h = {kps, desc, n, kf_kps, nkf, pose, nullptr, kp_has_point, npoints, points, point_desc, point_bad, nullptr,
                           nkf, kf_point, already_found};
    return pg_track_host(c, "bad argument to pgorb_search_by_projection_keyframe_pose", TRACK_KF, h, min_x, max_x, min_y, max_y, 0.0f, th, 0.0f,
                         orb_dist, check_orientation, nullptr, u, v, nullptr, dist3d, nullptr, nullptr, assigned);
}

int pgorb_search_by_projection_keyframe_pose_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, const int32_t* d_pair_kf,
        int npairs, float min_x, float max_x, float min_y, float max_y, const pgorb_kf_pose* d_pose, const uint8_t* d_kp_has_point,
        const int32_t* d_kf_point, const uint8_t* d_already_found, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
        const uint8_t* d_point_bad, float th, int orb_dist, int check_orientation, float* d_u, float* d_v, float* d_dist3d,
        int32_t* d_assigned, int32_t* d_nmatches, void* stream)
{
    const PgTrackCall t = {TRACK_KF, d_kps, d_n, cap_per_frame, d_pair_kf, nullptr, d_kp_has_point, cap_per_frame, nullptr, d_kf_point, d_already_found, 0.0f, th, 0.0f,
                           orb_dist, check_orientation, nullptr, d_u, d_v, nullptr, d_dist3d, nullptr, nullptr};
    return pg_track_batch(c, "bad argument to pgorb_search_by_projection_keyframe_pose_batch_device", d_kps, d_desc, d_n, cap_per_frame,
                          d_grid_start, d_grid_idx, d_pair_frame, npairs, min_x, max_x, min_y, max_y, d_pose, npoints, d_points, d_point_desc,
                          d_point_bad, nullptr, t, d_assigned, d_nmatches, (hipStream_t)stream);
}

}  // extern "C"
