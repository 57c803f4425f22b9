// kf_window.h -- what Fuse (fuse.hip) and loop closing's projection matchers (loop.hip) share: a map point projected into a key frame
// and the scan of the key frame's search window.  Included by those two translation units and, for kf_to_camera and kf_depth_ok,
// by the tracking thread's projection front (track.hip) and, for kf_row and kf_to_camera, by the Sim3Solver (sim3.hip).
//
// Restates (thirdparty/orb-slam2): the front part of ORBmatcher::Fuse (src/ORBmatcher.cc:856-897), repeated at :316-367, :1006-1058
// and :1152-1199, and KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:672-716).  Every float operation follows the
// reference's cv::Mat arithmetic under the readings of DESIGN.md section 4.
#pragma once
#include "match_common.h"

// key frames of ONE batch (keypoints, descriptors, grid indices `cap` apart, grid starts PGORB_GRID_CELLS + 1 apart), the map-point
// table, and the context's tables
struct PgKfBatch {
    const pgorb_keypoint* K; const uint8_t* D; const int32_t* n; int cap;
    const int32_t* gstart; const int32_t* gidx; const pgorb_kf_pose* pose;
    int npoints; const pgorb_map_point* pts; const uint8_t* pdesc; const uint8_t* pbad;
    float minX, minY, maxX, maxY;          // the key frame's int bounds (KeyFrame.h:195-198) as float
    float invW, invH;                      // mfGridElementWidthInv / HeightInv of the Frame's float bounds
    float sf[PG_MAXL + 1]; int nlevels; float logSf; float th;
};

static bool pg_kf_tables(pgorb_ctx* c, PgKfBatch& B, float min_x, float max_x, float min_y, float max_y, float th)
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

// The batch entry points' prologue, in the order a caller sees: the arguments -- `own` is the caller's check of its own, the shared
// ones are B's pointers and sizes, the bounds and th -- under the message `bad`, the 16 000 limit, the empty batch, the device and
// the tables.  true = return rc now.
static bool pg_kf_begin(pgorb_ctx* c, const char* bad, bool own, PgKfBatch& B, int nprob, float min_x, float max_x, float min_y,
                        float max_y, float th, int& rc)
{
    rc = PGORB_E_ARG;
    if (!c) return true;
    if (!own || !B.K || !B.D || !B.n || B.cap < 1 || !B.gstart || !B.gidx || nprob < 0 || B.npoints < 0 || !(max_x > min_x) ||
        !(max_y > min_y) || !(th > 0.0f) || (nprob && !B.pose) || (B.npoints && (!B.pts || !B.pdesc)))
        rc = pg_ctx_fail(c, PGORB_E_ARG, bad);
    else if (B.cap > 16000) rc = pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    else if (!nprob) rc = 0;
    else if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) rc = pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    else if (!pg_kf_tables(c, B, min_x, max_x, min_y, max_y, th)) rc = pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    else return false;
    return true;
}

// one row of R*p + t: gemm's small-matrix path with t as C
__device__ __forceinline__ float kf_row(const float* r, float t, const float* p)
{
    return cnm_f(__dadd_rn((double)cnm_dot3f(r[0], r[1], r[2], p[0], p[1], p[2]), (double)t));
}
// (a) world point -> camera point through a key frame's pose: p3Dc = Rcw*p3Dw + tcw
__device__ __forceinline__ void kf_to_camera(const pgorb_kf_pose& C, const float* pw, float* pc)
{
#pragma unroll
    for (int r = 0; r < 3; r++) pc[r] = kf_row(C.Tcw + 4 * r, C.Tcw[4 * r + 3], pw);
}

struct KfQuery { float u, v, r; int lvl, cx0, cx1, cy0, cy1; };
// (b) camera point pc -> the query of point P under C's intrinsics: positive depth, the projection, IsInImage, then depth(dist3D),
// which forms the point's distance and applies the caller's depth / viewing-angle tests at the reference's place (it runs only for
// a point inside the image), PredictScale, th*sf[level] and the cell window.  false = the reference `continue`s before the
// descriptor loop.
template <class Depth>
__device__ __forceinline__ bool kf_query(const PgKfBatch& B, const pgorb_kf_pose& C, const pgorb_map_point& P, const float* pc,
                                         Depth&& depth, KfQuery& Q)
{
    if (pc[2] < 0.0f) return false;
    const float invz = __fdiv_rn(1.0f, pc[2]);                       // (float)(1.0/z) in SearchBySim3: the double quotient rounds the same
    Q.u = __fadd_rn(__fmul_rn(C.fx, __fmul_rn(pc[0], invz)), C.cx);
    Q.v = __fadd_rn(__fmul_rn(C.fy, __fmul_rn(pc[1], invz)), C.cy);
    // IsInImage (KeyFrame.cc:713-716); `&`: one test of all four bounds, not a branch per coordinate with the bounds' loads behind it
    if (!((Q.u >= B.minX) & (Q.u < B.maxX) & (Q.v >= B.minY) & (Q.v < B.maxY))) return false;
    float dist3D;
    if (!depth(dist3D)) return false;
    Q.lvl = pg_predict_scale(P.max_distance, dist3D, B.logSf, B.nlevels);
    Q.r = __fmul_rn(B.th, B.sf[Q.lvl]);
    return sfi_window(Q.u, Q.v, Q.r, PgGridWin{B.minX, B.minY, B.invW, B.invH}, Q.cx0, Q.cx1, Q.cy0, Q.cy1);
}
// the depth test every form makes: dist3D inside [0.8*minDistance, 1.2*maxDistance]
__device__ __forceinline__ bool kf_depth_ok(const pgorb_map_point& P, float dist3D)
{
    return !(dist3D < __fmul_rn(0.8f, P.min_distance) || dist3D > __fmul_rn(1.2f, P.max_distance));
}

// Fuse's and the Scw forms' whole front part for table point mp and key frame f (:856-897, :316-367, :1006-1058): dist3D =
// cv::norm(PO) from the camera centre, and the viewing-angle test PO.dot(Pn) < 0.5*dist3D in double
__device__ __forceinline__ bool kf_point_query(const PgKfBatch& B, int f, int mp, KfQuery& Q)
{
    const pgorb_map_point P = B.pts[mp];                              // (a copy: all of the point is loaded at once, up front)
    const pgorb_kf_pose& C = B.pose[f];
    float pc[3];
    kf_to_camera(C, P.pos, pc);
    return kf_query(B, C, P, pc, [&](float& dist3D) {
        const float po0 = __fsub_rn(P.pos[0], C.Ow[0]), po1 = __fsub_rn(P.pos[1], C.Ow[1]), po2 = __fsub_rn(P.pos[2], C.Ow[2]);
        dist3D = cnm_f(cnm_normd(po0, po1, po2));
        return kf_depth_ok(P, dist3D) &&
               !(cnm_dotd(po0, po1, po2, P.normal[0], P.normal[1], P.normal[2]) < __dmul_rn(0.5, (double)dist3D)); }, Q);
}

// The window of Q over key frame f in the reference's (ix, iy, insertion) order: visit(idx, distance to point mp's descriptor) for
// every keypoint inside the radius whose octave lies in [level - 1, level] and that reject(idx, kp) lets through; returns whether
// vIndices was non-empty.  The octave and reject tests are pure `continue`s behind `any = true` and reject has no side effect, so
// their order cannot change a result; the octave goes first because a predicate may index a per-level table with it, and reject
// runs before the descriptor is read.  A grid entry outside [0, cap) is passed over.
template <class Reject, class Visit>
__device__ __forceinline__ bool kf_scan(const PgKfBatch& B, int f, int mp, const KfQuery& Q, Reject&& reject, Visit&& visit)
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
                const int o = kp.octave;
                if (o < Q.lvl - 1 || o > Q.lvl || o < 0) continue;
                if (reject(idx, kp)) continue;
                visit(idx, sfi_distance(q0, q1, D + (int64_t)idx * 32));
            }
        }
    return any;
}
