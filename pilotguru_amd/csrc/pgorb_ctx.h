// pgorb_ctx.h -- the inside of a context, for the host side of libpgorb.so only: api.hip (context, options, services),
// plan.hip (per-frame-size plan), extract.hip (launch order, extract entry points), stream.hip (pgorb_stream_*).
// No kernel file includes it: to them pgorb_ctx stays opaque behind the pg_ctx_* services of pgorb_internal.h.
#pragma once
#include "pgorb_internal.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

struct Arena { void* p = nullptr; size_t bytes = 0; };

struct pgorb_ctx {
    pgorb_params prm;
    double scaleFactor;                       // the reference keeps a double member
    float mvScaleFactor[PG_MAXL + 1], mvInvScaleFactor[PG_MAXL + 1];
    float mvLevelSigma2[PG_MAXL + 1], mvInvLevelSigma2[PG_MAXL + 1];
    int mnFeaturesPerLevel[PG_MAXL + 1];
    std::string err;
    // plan for the current frame size
    PgPlan plan;
    int planW = 0, planH = 0, planBatch = 0;
    bool planValid = false;
    // device memory
    Arena pyr, cand, sel, nodes, counters, tables, cellCand, cellCount, cellTab, cellTabBal, qtTab, qtLeaf;
    int qtThreads = 0;                        // K3 threads per workgroup: 0 = per launch (pgorb_set_option "quadtree_threads")
    int qtSplit = 2;                          // K3's candidate pass as its own launch: 0 no, 1 yes, 2 by frame size and batch (pgorb_set_option "quadtree_split")
    PgFusePlan fuse;                          // tables of the fused launches (make_plan)
    int fused = 0;                            // pgorb_set_option "fused_levels": 1 = resize + detect in one launch per level (fused.hip; measured slower, off by default)
    int fastTilePitch = 0, fastWpb = 1, fastCpw = PG_FAST_CPW_DEFAULT;       // K2 tile-shape sweep (pgorb_set_option "fast_tile_pitch" / "fast_waves_per_block")
    // K1 beside K2 (pgorb_set_option "pipeline_pyramid"): the pyramid chain on a high-priority side stream, K2 level by
    // level on a second one as the levels appear
    int pipePyr = 0;
    hipStream_t sPyr = nullptr, sFast = nullptr;
    hipEvent_t evFork = nullptr, evLevel[PG_MAXL] = {}, evPyrDone = nullptr, evFastDone = nullptr;
    // K3 / K4-6 of a group of levels beside K2 of the next group (pgorb_set_option "pipeline_levels", bit l = a group
    // starts at level l): K3 is one workgroup's critical path per (frame, level) and leaves the chip mostly idle
    int pipeLev = 0, pipeLevPrio = 0;
    hipStream_t sQt = nullptr, sDesc = nullptr;
    hipEvent_t evGrpFast[PG_MAXL] = {}, evGrpQt[PG_MAXL] = {}, evDescDone = nullptr;
    Arena stageA, stageOut, stageSfi, vocab;
    Arena xdesc;                              // matcher scratch: train descriptors as +-1 bytes (match.hip, match_mode 0 only)
    PgMatchOpts mx;                           // this context's matcher settings (pgorb_set_option "matcher" / "match_mode")
    void* pinned = nullptr;                   // page-locked bounce buffer for bulk result download
    size_t pinnedBytes = 0;
    Arena outBlk;                             // status word | counts | keypoints | descriptors of a host-frame call: one download
    double hostUs[4] = {0, 0, 0, 0}; int hostCalls = 0;
    // the host-frame calls run on a stream of the context's own, and replay their kernel chain (K1..K6 + the result download)
    // as a HIP graph from the second call with the same plan / batch size on (PGORB_EXTRACT_NO_GRAPH=1: direct launches)
    hipStream_t sHost = nullptr;
    int useGraph = 1, planEpoch = 0;
    struct HostGraph { hipGraph_t g = nullptr; hipGraphExec_t exec = nullptr; int nframes = 0, epoch = -1, seenFrames = 0, seenEpoch = -1; void* pinned = nullptr; size_t outBytes = 0; int last = 0; } hg;      // last: 0 direct, 1 captured, 2 replayed (pgorb_debug_host_graph)
    int vocabK = 0, vocabL = 0, vocabNodes = 0;
    int vocabScoring = 0, vocabWeighting = 0;  // the blob header's ScoringType / WeightingType (place.hip accepts L1_NORM with TF_IDF or TF)
    int lastFrames = 0;
    bool lastAliased = false;
    int lastFusedLaunches = 0;                // fused resize + detect launches the last batch issued (pgorb_get_option "fused_launches")
    // stage profiling (HIP events on the launch stream)
    std::vector<hipEvent_t> evExtract;        // 5 per armed extract call
    std::vector<hipEvent_t> evMatch;          // 2 per armed match call
    int profMax = 0, profExtract = 0, profMatch = 0;
    std::vector<pgorb_stream*> streams;       // live pgorb_stream_* objects of this context (pgorb_destroy takes them along)
    // the matchers' shared scratch arena (stageSfi) may be used from different caller streams: the last use is an event
    hipEvent_t evSfi = nullptr; hipStream_t sfiStream = nullptr; bool sfiUsed = false;
    // Sim3Solver's mRansacMaxIts as a function of N (pg_ctx_sim3_caps): the key it was made for and the device copy
    Arena sim3Caps;
    float sim3Prob = 0.0f; int sim3MinInliers = 0, sim3MaxIts = 0, sim3Entries = 0;
    // PnPsolver's adjusted mRansacMinInliers and mRansacMaxIts as a function of N (pg_ctx_pnp_table), kept the same way
    Arena pnpTable;
    float pnpProb = 0.0f, pnpEpsilon = 0.0f; int pnpMinInliers = 0, pnpMaxIts = 0, pnpMinSet = 0, pnpEntries = 0;
};

#pragma GCC visibility push(hidden)      // what follows is shared by the four host files, not exported

// api.hip
int fail(pgorb_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));      // c == NULL: pgorb_create's error
#define PG_HIP(c, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail((c), PGORB_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));   \
    } while (0)
int ensure(pgorb_ctx* c, Arena& a, size_t bytes);                               // a device arena of at least `bytes` (grows only)
void copy_tunables(pgorb_ctx* dst, pgorb_ctx* src);                             // every option of pgorb_set_option

// plan.hip
struct LevelGeom { int w, h, nCols, nRows, wCell, hCell, nIni; float hX; };
int level_geometry(const pgorb_ctx* c, int w, int h, LevelGeom* g);
int make_plan(pgorb_ctx* c, int w, int h, int nframes);

// extract.hip
int upright_size(pgorb_ctx* c, int rotate_degrees, int src_w, int src_h, int* w, int* h);
int run_batch(pgorb_ctx* c, const uint8_t* d_gray, bool resident_in_level0, int nframes, int w, int h, int stride, int64_t frame_stride,
              pgorb_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame, int32_t* d_n, hipStream_t s);
void destroy_side_streams(pgorb_ctx* c);

#pragma GCC visibility pop

// stream.hip: the sibling contexts of live multi-lane device streams follow pgorb_set_option
extern "C" void pg_forward_option_to_lanes(pgorb_ctx* c, const char* key, int value);
