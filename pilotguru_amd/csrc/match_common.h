// match_common.h -- what the Frame side, the guided matchers, CreateNewMapPoints, Fuse, loop closing's matchers and the map-point refresh
// share: included by frame.hip, init_match.hip (through cand_lists.h), window_match.hip (through proj_match.h, which includes
// cand_lists.h), node_match.hip, mapping.hip, fuse.hip, loop.hip (the last two through kf_window.h), track.hip (through kf_window.h
// and proj_match.h), sim3.hip (through kf_window.h), pose_opt.hip, initializer.hip, and map_point.hip, essential_graph.hip and
// loop_correct.hip (through loop_pose.h), and by no other translation unit.
#pragma once
#include "pgorb_internal.h"
#include <algorithm>
#include <string.h>
#include <vector>

#define GRID_COLS PGORB_GRID_COLS
#define GRID_ROWS PGORB_GRID_ROWS
#define GRID_CELLS PGORB_GRID_CELLS
#define HISTO_LENGTH 30         // ORBmatcher.cc:38-40
#define TH_LOW 50
#define TH_HIGH 100

// wave-wide inclusive sum / minimum on DPP row shifts and broadcasts (6 cross-lane moves on the VALU; the __shfl forms
// go through the LDS crossbar, ~100 cycles each, and the sequential matcher pass pays every one of them in full)
__device__ __forceinline__ int wave_incl_scan(int x, int lane)
{
    (void)lane;
    int v = x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31
    return v;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned x)
{
    int v = (int)x;                                                      // lanes a shift does not reach keep their own value
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));   // lane 15 of every row: the row's minimum
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane(v, 63);
}

// smallest and second-smallest of the lanes' (distinct or 0xFFFFFFFF) keys in ONE pass: every step merges two (min, second) pairs
__device__ __forceinline__ void wave_min2_u32(unsigned x, unsigned& best, unsigned& second)
{
    int a = (int)x, b = -1;                                              // (min, second) of the lanes seen so far; -1 = 0xFFFFFFFF
#define PG_MIN2_STEP(CTRL, ROWMASK) do { \
        const unsigned oa = (unsigned)__builtin_amdgcn_update_dpp(-1, a, CTRL, ROWMASK, 0xf, false); \
        const unsigned ob = (unsigned)__builtin_amdgcn_update_dpp(-1, b, CTRL, ROWMASK, 0xf, false); \
        const unsigned hi = max((unsigned)a, oa); \
        a = (int)min((unsigned)a, oa); \
        b = (int)min(min((unsigned)b, ob), hi); } while (0)
    PG_MIN2_STEP(0x111, 0xf); PG_MIN2_STEP(0x112, 0xf); PG_MIN2_STEP(0x114, 0xf); PG_MIN2_STEP(0x118, 0xf);
    PG_MIN2_STEP(0x142, 0xa); PG_MIN2_STEP(0x143, 0xc);
#undef PG_MIN2_STEP
    best = (unsigned)__builtin_amdgcn_readlane(a, 63);
    second = (unsigned)__builtin_amdgcn_readlane(b, 63);
}

// the dynamic LDS of every kernel of the family that asks for some
extern __shared__ __attribute__((aligned(16))) uint8_t pg_sfi_smem[];

// raises kernel K's dynamic LDS limit to `lds` on the context's device, once per device and size (one record per kernel)
template <auto K> static bool pg_raise_lds(pgorb_ctx* c, size_t lds)
{
    static size_t configured[64] = {0};
    const int dv = pg_ctx_device(c) & 63;
    if (lds > 160 * 1024) return false;
    if (lds > configured[dv]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        configured[dv] = lds;
    }
    return true;
}

// offsets of 256-byte aligned arrays inside one block of the matchers' scratch arena; `o` ends as the block's size
struct PgCarve {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; }
};

// the Frame's grid as GetFeaturesInArea sees it: mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv
struct PgGridWin { float minX, minY, invW, invH; };
// GetFeaturesInArea's cell window (Frame.cc:336-350); false = the reference returns an empty vector
__device__ __forceinline__ bool sfi_window(float x, float y, float r, const PgGridWin& G, int& cx0, int& cx1, int& cy0, int& cy1)
{
    const float minX = G.minX, minY = G.minY, invW = G.invW, invH = G.invH;
    cx0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, minX), r), invW)));
    if (cx0 >= PGORB_GRID_COLS) return false;
    cx1 = min(PGORB_GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, minX), r), invW)));
    if (cx1 < 0) return false;
    cy0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, minY), r), invH)));
    if (cy0 >= PGORB_GRID_ROWS) return false;
    cy1 = min(PGORB_GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, minY), r), invH)));
    if (cy1 < 0) return false;
    return cx1 >= cx0 && cy1 >= cy0;
}

// 256-bit Hamming distance of two descriptors held in registers / of one in registers and one in memory
__device__ __forceinline__ int pg_hamming256(const uint4 q0, const uint4 q1, const uint4 d0, const uint4 d1)
{
    return __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) +
           __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) + __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
}
__device__ __forceinline__ int sfi_distance(const uint4 q0, const uint4 q1, const uint8_t* d)
{
    return pg_hamming256(q0, q1, reinterpret_cast<const uint4*>(d)[0], reinterpret_cast<const uint4*>(d)[1]);
}

// cv::Mat arithmetic of the key-frame pose steps (CreateNewMapPoints, Fuse)
__device__ __forceinline__ float cnm_f(double x) { return __double2float_rn(x); }
// the small-matrix gemm path: t = a0*b0 + a1*b1 + a2*b2 in float, then (float)(t*1.0 + c*beta) in double
__device__ __forceinline__ float cnm_dot3f(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}
// Mat::dot / the squared L2 norm of CV_32F data: double sums from 0
__device__ __forceinline__ double cnm_dotd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = __dadd_rn(0.0, __dmul_rn((double)a0, (double)b0));
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b1));
    return __dadd_rn(s, __dmul_rn((double)a2, (double)b2));
}
__device__ __forceinline__ double cnm_normd(float a0, float a1, float a2) { return __dsqrt_rn(cnm_dotd(a0, a1, a2, a0, a1, a2)); }
// MapPoint::PredictScale(currentDist, Frame*) (MapPoint.cc:516-531); (int)ceil(...) of a NaN / out-of-range value is what
// x86-64's cvttss2si returns, INT_MIN, i.e. level 0 after the clamp
__host__ __device__ inline int pg_predict_scale(float maxDistance, float currentDist, float logScaleFactor, int nlevels)
{
#ifdef __HIP_DEVICE_COMPILE__
    const float ratio = __fdiv_rn(maxDistance, currentDist);
    const float q = ceilf(__fdiv_rn(pg_log_f(ratio), logScaleFactor));
#else
    const float ratio = maxDistance / currentDist;
    const float q = ceilf(pg_log_f(ratio) / logScaleFactor);
#endif
    int nScale = (q != q || q >= 2147483648.0f || q < -2147483648.0f) ? (-2147483647 - 1) : (int)q;
    if (nScale < 0) nScale = 0;
    else if (nScale >= nlevels) nScale = nlevels - 1;
    return nScale;
}

// rotation-histogram bin of a match: the angle difference in [0, 360) times 1/HISTO_LENGTH, rounded (ORBmatcher.cc:473-483)
__device__ __forceinline__ int pg_rot_bin(float qangle, float kangle)
{
    float rot = __fsub_rn(qangle, kangle);                            // also :241-250, :1428-1434
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cc:1605-1646) over the HISTO_LENGTH bin sizes binSize(0), binSize(1), ...: the indices of the three
// largest bins, the first of equal ones winning, and -1 for a second / third below a tenth of the largest
template <class F> __device__ __forceinline__ void pg_three_maxima(F&& binSize, int& out1, int& out2, int& out3)
{
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;     // (locals: updated through the references they end up in scratch memory)
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = binSize(i);
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    out1 = ind1; out2 = ind2; out3 = ind3;
}

// ---- the BoW-node matchers' batch (node_match.hip), built by mapping.hip too ----
// Frames of ONE extract batch: keypoints, descriptors and fvNode / fvFeat `cap` apart, fvStart cap + 1 apart; the FeatureVectors are
// the per-frame CSR arrays k_feature_vectors builds on the device.
struct PgFvBatch {
    const pgorb_keypoint* K; const uint8_t* D; const int32_t* n; int cap;
    const uint32_t* fvNode; const int32_t* fvStart; const uint32_t* fvFeat; const int32_t* nfv;
};
struct PgTriBatch {
    PgFvBatch fv;
    const int32_t* pairKF1; const int32_t* pairKF2; const float* F12; const float* epipole;
    const uint8_t* hasPoint2;              // [npairs][cap] (a zeroed scratch array when the caller passes none)
    float epiTh[PG_MAXL + 1];              // 100*mvScaleFactors[octave] (float, :749)
    double lineTh[PG_MAXL + 1];            // 3.84*mvLevelSigma2[octave] (double, :158)
};
// SearchForTriangulation's launches on `stream` (its batch entry and CreateNewMapPoints): the per-octave thresholds of T, clear the
// outputs, the node pass, the finishing pass; bins = [npairs][cap] i8 scratch
int pg_tri_launch(pgorb_ctx* c, PgTriBatch T, int npairs, const uint8_t* d_has_point1, int check_orientation, int32_t* d_matches12,
                  int8_t* bins, int32_t* d_nmatches, hipStream_t stream);

// a FeatureVector as CSR: starts from 0, ascending, inside n, every feature index below n
bool pg_fv_ok(const int32_t* start, const uint32_t* feat, int nfv, int n);

// One frame of a single host call of a BoW-node matcher (SearchByBoW, SearchForTriangulation, CreateNewMapPoints)
struct PgFvFrame {
    const pgorb_keypoint* kps;   // null: zero keypoints that carry `angle` only
    const float* angle;
    const uint8_t* desc;
    const uint8_t* mask;         // null: all zero
    int n;
    const uint32_t* node; const int32_t* start; const uint32_t* feat; int nfv;
};
// ... and `nframes` of them as the uploads of one batch (frame 0, frame 1, ...): keypoints, descriptors, masks and FeatureVectors in
// slots of cap = max(n, 1) entries (cap + 1 starts), the tail of every slot zero; n[nframes], nfv[nframes] and the frame numbers
// P = {0, 1, ...} for the pair and neighbour lists to point into.  The FeatureVector arrays are read up to start[nfv] only.
struct PgFvPack {
    int nframes, cap;
    size_t K, D, H, N, FN, FS, FF, NF, P;
    PgFvPack(PgHostCall& s, const PgFvFrame* f, int nframes);
    void pack(PgHostCall& s, const PgFvFrame* f) const;
};

// One key frame of a single host call of a projection matcher (Fuse, the Scw forms, SearchBySim3); slots null: every slot empty
struct PgKfFrame { const pgorb_keypoint* kps; const uint8_t* desc; const int32_t* slots; const pgorb_kf_pose* pose; int n; };
// ... and `nframes` of them as one batch: keypoints, descriptors and slot rows (filled with -1 past n) in slots of cap = max(n, 1)
// entries, the poses, n[nframes] and the frame numbers F = {0, 1, ...}; the map-point table (points, descriptors, bad mask) in
// max(npoints, 1) entries; and, declared by device() after the caller's own uploads and downloads, the two grid arrays grid() fills.
struct PgKfPack {
    int nframes, cap, npoints;
    size_t K, D, S, Pose, N, F, P, PD, B, GS, GI;
    PgKfPack(PgHostCall& s, const PgKfFrame* f, int nframes, int npoints);
    void device(PgHostCall& s);
    void pack(PgHostCall& s, const PgKfFrame* f, const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad) const;
    int grid(pgorb_ctx* c, PgHostCall& s, float min_x, float max_x, float min_y, float max_y) const;      // the frames' grids, on the null stream
};
