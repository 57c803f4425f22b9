// proj_match.h -- what the projection matchers given their projections (window_match.hip) and the tracking thread's matchers that
// project on the device (track.hip) share: the query arrays the two passes of SearchByProjection read, the family's LDS limit and the
// launch of the two passes; the candidate lists between the passes are cand_lists.h.  Included by those two translation units only.
#pragma once
#include "cand_lists.h"

// Batch layout of SearchByProjection's two passes (k_proj_candidates, k_search_by_projection; window_match.hip): pair p matches its
// nq[p] queries against frame pairFrame[p] of an extract batch (keypoints / descriptors `cap` apart, grids (GRID_CELLS + 1) / cap
// apart); query arrays are [npairs][qcap].
struct PgProjBatch {
    const pgorb_keypoint* K; const uint8_t* D; const int32_t* n; int cap;
    const int32_t* gstart; const int32_t* gidx; const int32_t* pairFrame;
    const uint8_t* kpHasPoint;             // [npairs][cap] or null
    int qcap; const int32_t* nq;
    const uint8_t* valid; const float* x; const float* y; const int32_t* level; const float* aux;   // aux: view cos (mode 0) / angle (mode 1)
    const uint8_t* desc; const uint8_t* hasObs;
    float sf[PG_MAXL + 1]; int nlevels; float th;
    // mode 2 (key frame, relocalisation): level = PredictScale(dist3d), aux = the key frame keypoint's angle
    const uint8_t* found; const float* dist3d; const float* minDist; const float* maxDist; float logSf; int orbDist;
    float maxX, maxY;                      // mnMaxX / mnMaxY (the kernels derive everything else from minX / minY and the inverse cell sizes)
};

// The dynamic LDS of k_search_by_projection for `cap` keypoints and `qcap` queries: minq, minAny, asg (4 B each) and taken (1 B) per
// keypoint; listA, listB, cntL, qBest (2 B each), rotBin and done (1 B each) per query; the counters and the histogram.  This line, not
// the 16 000 of the other matchers, is the family's limit: 12 582 keypoints with one query, 7 112 with as many queries, 16 358 queries
// with one keypoint (the 16 000 gate comes first there).
static size_t pg_sbp_lds(int cap, int qcap) { return (size_t)cap * 13 + (size_t)qcap * 10 + 256; }
static const size_t PG_SBP_LDS_MAX = (size_t)160 * 1024;      // what pg_raise_lds grants a workgroup (match_common.h)
static const char* const PG_SBP_LDS_MSG =
    "SearchByProjection: keypoints * 13 + queries * 10 + 256 bytes exceed the 163840 B of LDS (e.g. 12582 keypoints with 1 query, 7112 with 7112)";

// what the key-frame form (mode 2) takes beyond the common query arrays
struct PgProjKeyFrame { const uint8_t* found; const float* dist3d; const float* minDist; const float* maxDist; float logSf; int orbDist; };

// The two passes behind a front part that fills the query arrays on the device.  pg_proj_begin: the family's LDS limit for `cap`
// keypoints and `qcap` queries a pair (neither above LIST_MAX_N: the caller's check, asserted here), the device, and ONE block of the
// matchers' scratch arena holding the candidate lists of npairs x qcap queries and, behind them, `extraBytes` for the caller's own
// arrays (*extra, 256-byte aligned).  pg_proj_run: pass A, pass B and the arena's event, on `stream`; B's sf / nlevels are filled here.
int pg_proj_begin(pgorb_ctx* c, int cap, int qcap, int npairs, size_t extraBytes, hipStream_t stream, PgLists* Ls, void** extra);
int pg_proj_run(pgorb_ctx* c, PgProjBatch& B, int npairs, float min_x, float max_x, float min_y, float max_y, int mode, float nnratio,
                int check_orientation, const PgLists& Ls, int32_t* d_assigned, int32_t* d_nmatches, hipStream_t stream);
