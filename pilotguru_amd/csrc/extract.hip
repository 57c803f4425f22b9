// extract.hip -- the launch order of K1..K6 (ORBextractor::operator() sequencing, thirdparty/orb-slam2/src/ORBextractor.cc:1042-1104)
// with its three alternate orders, and the entry points that run it: pgorb_extract*, their status check, profiling, stage taps.
#include "pgorb_ctx.h"

#include <chrono>

namespace {

// The side streams of the pipeline options: two priority streams and a set of untimed events each, made by the first batch
// that runs with the option on.  Each set's events are listed once; making and destroying both walk that list.
std::vector<hipEvent_t*> pipe_pyr_events(pgorb_ctx* c)      // "pipeline_pyramid": sPyr (high priority), sFast
{
    std::vector<hipEvent_t*> v{&c->evFork, &c->evPyrDone, &c->evFastDone};
    for (hipEvent_t& e : c->evLevel) v.push_back(&e);
    return v;
}
std::vector<hipEvent_t*> pipe_lev_events(pgorb_ctx* c)      // "pipeline_levels": sQt ("pipeline_levels_priority": high), sDesc
{
    std::vector<hipEvent_t*> v{&c->evDescDone};
    for (hipEvent_t& e : c->evGrpFast) v.push_back(&e);
    for (hipEvent_t& e : c->evGrpQt) v.push_back(&e);
    return v;
}
int make_side_streams(pgorb_ctx* c, hipStream_t* a, bool aHigh, hipStream_t* b, const std::vector<hipEvent_t*>& events)
{
    int lo = 0, hi = 0;
    PG_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    PG_HIP(c, hipStreamCreateWithPriority(a, hipStreamNonBlocking, aHigh ? hi : lo));
    PG_HIP(c, hipStreamCreateWithPriority(b, hipStreamNonBlocking, lo));
    for (hipEvent_t* e : events) PG_HIP(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return 0;
}
void drop_side_streams(hipStream_t a, hipStream_t b, const std::vector<hipEvent_t*>& events)
{
    if (!a) return;
    (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
    (void)hipStreamDestroy(a); (void)hipStreamDestroy(b);
    for (hipEvent_t* e : events) (void)hipEventDestroy(*e);
}

}  // namespace

void destroy_side_streams(pgorb_ctx* c)
{
    drop_side_streams(c->sPyr, c->sFast, pipe_pyr_events(c));
    drop_side_streams(c->sQt, c->sDesc, pipe_lev_events(c));
}

// PGORB_DEBUG_SYNC=1: wait behind every kernel of the one-launch-per-kernel path and say which one completed (a GPU memory fault
// then names its kernel: the last line printed is the kernel BEFORE the faulting one)
#define PG_DBG_SYNC(name) do { static const bool dbg_ = getenv("PGORB_DEBUG_SYNC") != nullptr; \
                               if (dbg_) { (void)hipStreamSynchronize(s); fprintf(stderr, "[pgorb] %s done (%dx%d x %d)\n", name, w, h, nframes); fflush(stderr); } } while (0)
int run_batch(pgorb_ctx* c, const uint8_t* d_gray, bool resident_in_level0, int nframes, int w, int h,
              int stride, int64_t frame_stride, pgorb_keypoint* d_kps, uint8_t* d_desc,
              int cap_per_frame, int32_t* d_n, hipStream_t s)
{
    PgPlan P = c->plan;                                   // by-value copy handed to the kernels, with the context's tunables
    P.fastTilePitch = c->fastTilePitch; P.fastWpb = c->fastWpb; P.fastCpw = c->fastCpw; P.qtSplit = c->qtSplit; P.qtThreads = c->qtThreads;
    c->lastAliased = false;
    c->lastFusedLaunches = 0;
    if (!resident_in_level0) {
        const bool aligned = ((uintptr_t)d_gray % 4 == 0) && (stride % 4 == 0) && (frame_stride % 4 == 0);
        if (aligned) {                                    // zero-copy: level 0 is the caller's buffer
            P.lvl[0].img = const_cast<uint8_t*>(d_gray);
            P.lvl[0].pitch = stride;
            P.lvl[0].fstride = frame_stride;
            c->lastAliased = true;
        } else {
            pg_launch_copy_level0(P, d_gray, stride, frame_stride, nframes, s);
        }
    }
    // the device status word is per batch: cleared by the first pyramid launch (pyramid.hip) where the order of the kernels allows it,
    // by a memset otherwise
    const bool fusedPath = c->fused && !c->pipePyr && !c->pipeLev && P.nlevels > 1;
    const bool foldClear = !c->pipePyr && P.nlevels > 1 && !fusedPath;
    if (!foldClear) PG_HIP(c, hipMemsetAsync(P.status, 0, 16, s));
    hipEvent_t* ev = (c->profExtract < c->profMax) ? &c->evExtract[5 * (size_t)c->profExtract] : nullptr;
    if (ev) PG_HIP(c, hipEventRecord(ev[0], s));
    if (c->pipePyr && P.nlevels > 1) {
        // K1 is HBM-bound and K2 VALU-issue-bound, and K2 of level l only needs level l: the resize chain runs on a
        // high-priority side stream, K2 level by level on another, each level's K2 behind the launch that wrote it.
        // (Stage events: "pyramid" = start .. end of the chain, "fast" = end of the chain .. end of K2: they overlap.)
        if (int rc = c->sPyr ? 0 : make_side_streams(c, &c->sPyr, true, &c->sFast, pipe_pyr_events(c))) return rc;
        PG_HIP(c, hipEventRecord(c->evFork, s));
        PG_HIP(c, hipStreamWaitEvent(c->sPyr, c->evFork, 0));
        PG_HIP(c, hipStreamWaitEvent(c->sFast, c->evFork, 0));
        pg_launch_fast_levels(P, nframes, 0, 1, c->sFast);
        for (int l = 1; l < P.nlevels; l++) {
            pg_launch_pyramid_level(P, l, nframes, c->sPyr);
            PG_HIP(c, hipEventRecord(c->evLevel[l], c->sPyr));
            PG_HIP(c, hipStreamWaitEvent(c->sFast, c->evLevel[l], 0));
            pg_launch_fast_levels(P, nframes, l, l + 1, c->sFast);
        }
        PG_HIP(c, hipEventRecord(c->evPyrDone, c->sPyr));
        PG_HIP(c, hipEventRecord(c->evFastDone, c->sFast));
        PG_HIP(c, hipStreamWaitEvent(s, c->evPyrDone, 0));
        if (ev) PG_HIP(c, hipEventRecord(ev[1], s));
        PG_HIP(c, hipStreamWaitEvent(s, c->evFastDone, 0));
        if (ev) PG_HIP(c, hipEventRecord(ev[2], s));
    } else if (c->pipeLev && P.nlevels > 1) {
        // K2 group by group on the caller's stream; K3 of a group on a second stream as soon as its K2 is done, K4-6 of a
        // group on a third as soon as its K3 is done: the latency-bound quadtree of one group runs under the issue-bound
        // kernels of the others.  (Stage events: "fast" = K2 of all groups, "quadtree" = the wait for the side streams.)
        if (int rc = c->sQt ? 0 : make_side_streams(c, &c->sQt, c->pipeLevPrio != 0, &c->sDesc, pipe_lev_events(c))) return rc;
        for (int l = 1; l < P.nlevels; l++)
            if (!pg_launch_pyramid_level(P, l, nframes, s, l == 1 ? P.status : nullptr) && l == 1) PG_HIP(c, hipMemsetAsync(P.status, 0, 16, s));
        if (ev) PG_HIP(c, hipEventRecord(ev[1], s));
        for (int beg = 0; beg < P.nlevels;) {
            int end = beg + 1;
            while (end < P.nlevels && !((c->pipeLev >> end) & 1)) end++;
            pg_launch_fast_levels(P, nframes, beg, end, s);
            PG_HIP(c, hipEventRecord(c->evGrpFast[beg], s));
            PG_HIP(c, hipStreamWaitEvent(c->sQt, c->evGrpFast[beg], 0));
            pg_launch_quadtree_levels(P, nframes, beg, end, c->sQt);
            PG_HIP(c, hipEventRecord(c->evGrpQt[beg], c->sQt));
            PG_HIP(c, hipStreamWaitEvent(c->sDesc, c->evGrpQt[beg], 0));
            if (!pg_launch_describe_levels(P, nframes, d_kps, d_desc, cap_per_frame, d_n, beg, end, c->sDesc)) return fail(c, PGORB_E_HIP, "K4-6: the Gaussian taps derived on this host differ from the kernel's compiled-in constants");
            beg = end;
        }
        if (ev) PG_HIP(c, hipEventRecord(ev[2], s));
        PG_HIP(c, hipEventRecord(c->evDescDone, c->sDesc));
        PG_HIP(c, hipStreamWaitEvent(s, c->evDescDone, 0));
        if (ev) { PG_HIP(c, hipEventRecord(ev[3], s)); PG_HIP(c, hipEventRecord(ev[4], s)); c->profExtract++; }
        PG_HIP(c, hipGetLastError());
        c->lastFrames = nframes;
        return 0;
    } else if (c->fused && P.nlevels > 1) {
        // Every level read ONCE (fused.hip): the launch that resizes level l -> l + 1 detects level l; a level without fused tables
        // takes K1 + its own K2; the last level is detected by K2.  (Stage events: "pyramid" = the chain of fused launches, i.e. the
        // whole pyramid AND the detection of levels 0 .. L-2; "fast" = what is left for K2.)
        PG_HIP(c, hipMemsetAsync(P.status, 0, 16, s));        // (K2's part of the first launch may report: the word is cleared in front of it)
        int pending = -1;                                     // first level of a run of levels still waiting for K2
        for (int l = 0; l + 1 < P.nlevels; l++) {
            if (pg_launch_pyr_fast(P, c->fuse, l, nframes, s)) {
                c->lastFusedLaunches++;
                if (pending >= 0) { pg_launch_fast_levels(P, nframes, pending, l, s); pending = -1; }
            } else {
                pg_launch_pyramid_level(P, l + 1, nframes, s);
                if (pending < 0) pending = l;
            }
        }
        if (ev) PG_HIP(c, hipEventRecord(ev[1], s));
        pg_launch_fast_levels(P, nframes, pending >= 0 ? pending : P.nlevels - 1, P.nlevels, s);
        if (ev) PG_HIP(c, hipEventRecord(ev[2], s));
    } else {
        for (int l = 1; l < P.nlevels; l++) {
            if (!pg_launch_pyramid_level(P, l, nframes, s, l == 1 ? P.status : nullptr) && l == 1) PG_HIP(c, hipMemsetAsync(P.status, 0, 16, s));
            PG_DBG_SYNC("K1 pyramid level");
        }
        if (ev) PG_HIP(c, hipEventRecord(ev[1], s));
        pg_launch_fast(P, nframes, s);
        PG_DBG_SYNC("K2 fast");
        if (ev) PG_HIP(c, hipEventRecord(ev[2], s));
    }
    pg_launch_quadtree(P, nframes, s);
    PG_DBG_SYNC("K3 quadtree");
    if (ev) PG_HIP(c, hipEventRecord(ev[3], s));
    if (!pg_launch_describe(P, nframes, d_kps, d_desc, cap_per_frame, d_n, s)) return fail(c, PGORB_E_HIP, "K4-6: the Gaussian taps derived on this host differ from the kernel's compiled-in constants");
    PG_DBG_SYNC("K4-6 describe");
    if (ev) { PG_HIP(c, hipEventRecord(ev[4], s)); c->profExtract++; }
    PG_HIP(c, hipGetLastError());
    c->lastFrames = nframes;
    return 0;
}

// the upright size of src_w x src_h frames turned by `rot` degrees (image_sequence_reader.cc:203-207)
int upright_size(pgorb_ctx* c, int rot, int src_w, int src_h, int* w, int* h)
{
    if (rot != 0 && rot != 90 && rot != 180 && rot != 270) return fail(c, PGORB_E_ARG, "unsupported rotation %d: only multiples of 90 degrees", rot);
    const bool swap = rot == 90 || rot == 270;
    *w = swap ? src_h : src_w; *h = swap ? src_w : src_h;
    return 0;
}

// what a batch's device status word says (0: nothing)
static int device_status(pgorb_ctx* c, int32_t st)
{
    if (!st) return 0;
    return fail(c, st, st == PGORB_E_TOOSMALL ? "device status %d (a pyramid level more than twice as tall as wide has candidates: the reference divides by zero there)"
                                              : "device status %d (internal candidate capacity exceeded)", st);
}

extern "C" {

int pgorb_extract(pgorb_ctx* c, const uint8_t* gray, int w, int h, int stride, pgorb_keypoint* kps,
                  uint8_t* desc, int cap, int* n)
{
    const uint8_t* frames[1] = {gray};
    if (c && n && (!gray || w <= 0 || h <= 0)) { *n = 0; return 0; }       // :1045
    return pgorb_extract_batch(c, frames, 1, w, h, stride, kps, desc, cap, n);
}

// Frames in host memory, results to host memory: the reference's call shape (ORBextractor::operator() on a pageable cv::Mat,
// one frame per synchronous call: Frame.cc:251-257, Tracking.cc:262-266).  Round 4 cut the call's fixed costs:
//   * input: hipMemcpy2DAsync straight from the caller's (pageable) memory.  A page-locked staging buffer of the context's own,
//     filled in row chunks while the DMA engine moves the previous chunk, measured 24 us SLOWER per 1080p frame than the
//     runtime's pageable path (each extra copy command costs more than the overlap saves);
//   * output: status word, counts, keypoints and descriptors live in ONE device block (PgPlan::status points into it) and come
//     back with one download and one synchronisation (there were two synchronous 4-byte copies in front of it).
// Host phases of the last calls: pgorb_profile_host.
int pgorb_extract_batch(pgorb_ctx* c, const uint8_t* const* gray, int nframes, int w, int h,
                        int stride, pgorb_keypoint* kps, uint8_t* desc, int cap, int* n)
{
    if (!c) return PGORB_E_ARG;
    if (!n) return fail(c, PGORB_E_ARG, "null count pointer");
    for (int f = 0; f < nframes; f++) n[f] = 0;
    if (nframes < 1 || !gray) return fail(c, PGORB_E_ARG, "bad argument to pgorb_extract_batch");
    if (w <= 0 || h <= 0) return 0;          // empty image: the reference returns silently (:1045)
    if (!kps || !desc || cap < 1 || stride < w) return fail(c, PGORB_E_ARG, "bad argument to pgorb_extract_batch");
    const auto t0 = std::chrono::steady_clock::now();
    int rc = make_plan(c, w, h, nframes);
    if (rc) return rc;
    for (int f = 0; f < nframes; f++) if (!gray[f]) return fail(c, PGORB_E_ARG, "null frame %d", f);
    const int need = c->plan.selTotal;       // the device block always holds the full bound
    // device result block of this call: status (64 B) | n[nframes] | kps[nframes][need] | desc[nframes][need][32]
    auto al64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
    const size_t oN = 64, oK = oN + al64((size_t)nframes * 4), oD = oK + al64((size_t)nframes * need * sizeof(pgorb_keypoint)),
                 outBytes = oD + (size_t)nframes * need * 32;
    uint8_t* blk = (uint8_t*)c->outBlk.p;    // (make_plan sized it for max_batch frames)
    void* hv;
    if ((rc = pg_ctx_pinned(c, outBytes, &hv))) return rc;
    if (!c->sHost) PG_HIP(c, hipStreamCreateWithFlags(&c->sHost, hipStreamNonBlocking));
    hipStream_t hs = c->sHost;
    // ---- upload ----
    const PgLevel& L0 = c->plan.lvl[0];
    for (int f = 0; f < nframes; f++)
        PG_HIP(c, hipMemcpy2DAsync(L0.img + (int64_t)f * L0.fstride, L0.pitch, gray[f], stride, w, h, hipMemcpyHostToDevice, hs));
    const auto t1 = std::chrono::steady_clock::now();
    // ---- kernels ----
    // Direct launches the first time a (plan, batch size) is seen -- the launchers may still allocate or configure --, captured
    // into a graph the second time, replayed from then on: the 10 launches + the download become one submission (the 7 resize
    // launches of a single frame are launch-bound: ~5 us apiece for ~2 us of work).  Not while a profile is armed (its events
    // would be captured) or a multi-stream pipeline option is on.
    pgorb_ctx::HostGraph& G = c->hg;
    const bool graphable = c->useGraph && c->profExtract >= c->profMax && !c->pipePyr && !c->pipeLev;
    const bool replay = graphable && G.exec && G.nframes == nframes && G.epoch == c->planEpoch && G.pinned == hv && G.outBytes == outBytes;
    auto launch = [&] { return run_batch(c, nullptr, true, nframes, w, h, stride, 0, (pgorb_keypoint*)(blk + oK), blk + oD, need, (int32_t*)(blk + oN), hs); };
    bool graph = replay;
    G.last = replay ? 2 : 0;
    if (!replay) {
        const bool capture = graphable && G.seenFrames == nframes && G.seenEpoch == c->planEpoch;
        G.seenFrames = nframes; G.seenEpoch = c->planEpoch;
        if (capture) {
            PG_HIP(c, hipStreamBeginCapture(hs, hipStreamCaptureModeRelaxed));
            rc = launch();
            const hipError_t e1 = rc ? hipSuccess : hipMemcpyAsync(hv, blk, outBytes, hipMemcpyDeviceToHost, hs);
            hipGraph_t g = nullptr;
            const hipError_t e2 = hipStreamEndCapture(hs, &g);
            if (!rc && e1 == hipSuccess && e2 == hipSuccess && g) {
                if (G.exec) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
                if (G.g) { (void)hipGraphDestroy(G.g); G.g = nullptr; }
                hipGraphExec_t ex = nullptr;
                graph = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess;
                if (graph) { G.g = g; G.exec = ex; G.nframes = nframes; G.epoch = c->planEpoch; G.pinned = hv; G.outBytes = outBytes; G.last = 1; }
            }
            if (!graph) {
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                c->useGraph = 0;                               // capture or instantiation failed: direct launches, now and from here on
                if (rc) return rc;
            }
        }
    }
    if (graph) {
        PG_HIP(c, hipGraphLaunch(G.exec, hs));
        c->lastFrames = nframes; c->lastAliased = false;
    } else {
        if ((rc = launch())) return rc;
        const hipError_t e1 = hipMemcpyAsync(hv, blk, outBytes, hipMemcpyDeviceToHost, hs);
        if (e1 != hipSuccess) return fail(c, PGORB_E_HIP, "hipMemcpyAsync D2H failed: %s", hipGetErrorString(e1));
    }
    const auto t2 = std::chrono::steady_clock::now();
    PG_HIP(c, hipStreamSynchronize(hs));
    const auto t3 = std::chrono::steady_clock::now();
    // ---- results ----
    const uint8_t* hb = (const uint8_t*)hv;
    const int32_t st = *(const int32_t*)hb;
    if (st) return device_status(c, st);
    const int32_t* cnt = (const int32_t*)(hb + oN);
    for (int f = 0; f < nframes; f++)
        if (cnt[f] > cap)
            return fail(c, PGORB_E_CAP, "frame %d has %d keypoints, capacity %d", f, cnt[f], cap);
    for (int f = 0; f < nframes; f++) {
        n[f] = cnt[f];
        if (!cnt[f]) continue;
        memcpy(kps + (size_t)f * cap, hb + oK + (size_t)f * need * sizeof(pgorb_keypoint), (size_t)cnt[f] * sizeof(pgorb_keypoint));
        memcpy(desc + (size_t)f * cap * 32, hb + oD + (size_t)f * need * 32, (size_t)cnt[f] * 32);
    }
    const auto t4 = std::chrono::steady_clock::now();
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    c->hostUs[0] += us(t0, t1); c->hostUs[1] += us(t1, t2); c->hostUs[2] += us(t2, t3); c->hostUs[3] += us(t3, t4); c->hostCalls++;
    return 0;
}

int pgorb_extract_batch_device(pgorb_ctx* c, const uint8_t* d_gray, int nframes, int w, int h,
                               int stride, int64_t frame_stride, pgorb_keypoint* d_kps,
                               uint8_t* d_desc, int cap_per_frame, int32_t* d_n, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_gray || !d_kps || !d_desc || !d_n || nframes < 1 || w < 1 || h < 1 || stride < w ||
        cap_per_frame < 1)
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_extract_batch_device");
    if (int rc = make_plan(c, w, h, nframes)) return rc;
    return run_batch(c, d_gray, false, nframes, w, h, stride, frame_stride, d_kps, d_desc,
                     cap_per_frame, d_n, (hipStream_t)stream);
}

int pgorb_extract_batch_color_device(pgorb_ctx* c, const uint8_t* d_img, int nframes, int w, int h, int stride,
                                     int64_t frame_stride, int channels, int rgb_order, pgorb_keypoint* d_kps,
                                     uint8_t* d_desc, int cap_per_frame, int32_t* d_n, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_img || !d_kps || !d_desc || !d_n || nframes < 1 || w < 1 || h < 1 || (channels != 3 && channels != 4) ||
        stride < w * channels || cap_per_frame < 1)
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_extract_batch_color_device");
    if (int rc = make_plan(c, w, h, nframes)) return rc;
    pg_launch_color_to_gray(c->plan, d_img, stride, frame_stride, channels, rgb_order, nframes, (hipStream_t)stream);
    return run_batch(c, nullptr, true, nframes, w, h, w, 0, d_kps, d_desc, cap_per_frame, d_n, (hipStream_t)stream);
}

int pgorb_extract_batch_ingest_device(pgorb_ctx* c, const uint8_t* d_img, int nframes, int src_w, int src_h, int stride,
                                      int64_t frame_stride, int channels, int rgb_order, int rotate_degrees,
                                      int vertical_flip, int horizontal_flip, pgorb_keypoint* d_kps, uint8_t* d_desc,
                                      int cap_per_frame, int32_t* d_n, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_img || !d_kps || !d_desc || !d_n || nframes < 1 || src_w < 1 || src_h < 1 ||
        (channels != 1 && channels != 3 && channels != 4) || stride < src_w * channels || cap_per_frame < 1)
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_extract_batch_ingest_device");
    int w, h, rc;
    if ((rc = upright_size(c, rotate_degrees, src_w, src_h, &w, &h)) || (rc = make_plan(c, w, h, nframes))) return rc;
    pg_launch_ingest(c->plan, d_img, stride, frame_stride, src_w, src_h, channels, rgb_order, rotate_degrees / 90,
                     vertical_flip != 0, horizontal_flip != 0, nframes, (hipStream_t)stream);
    return run_batch(c, nullptr, true, nframes, w, h, w, 0, d_kps, d_desc, cap_per_frame, d_n, (hipStream_t)stream);
}

int pgorb_check_async(pgorb_ctx* c, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!c->planValid) return 0;
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipStreamSynchronize((hipStream_t)stream));
    int32_t st = 0;
    PG_HIP(c, hipMemcpy(&st, c->plan.status, 4, hipMemcpyDeviceToHost));
    return device_status(c, st);
}

int pgorb_profile_begin(pgorb_ctx* c, int max_calls)
{
    if (!c || max_calls < 0) return PGORB_E_ARG;
    PG_HIP(c, hipSetDevice(c->prm.device));
    while ((int)c->evExtract.size() < 5 * max_calls) {
        hipEvent_t e; PG_HIP(c, hipEventCreate(&e)); c->evExtract.push_back(e);
    }
    while ((int)c->evMatch.size() < 2 * max_calls) {
        hipEvent_t e; PG_HIP(c, hipEventCreate(&e)); c->evMatch.push_back(e);
    }
    c->profMax = max_calls; c->profExtract = 0; c->profMatch = 0;
    return 0;
}

int pgorb_profile_read(pgorb_ctx* c, double* ms)
{
    if (!c || !ms) return PGORB_E_ARG;
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipDeviceSynchronize());
    for (int i = 0; i < PGORB_NSTAGES; i++) ms[i] = 0;
    for (int k = 0; k < c->profExtract; k++)
        for (int st = 0; st < 4; st++) {
            float t = 0;
            PG_HIP(c, hipEventElapsedTime(&t, c->evExtract[5 * (size_t)k + st], c->evExtract[5 * (size_t)k + st + 1]));
            ms[st] += t;
        }
    for (int k = 0; k < c->profMatch; k++) {
        float t = 0;
        PG_HIP(c, hipEventElapsedTime(&t, c->evMatch[2 * (size_t)k], c->evMatch[2 * (size_t)k + 1]));
        ms[4] += t;
    }
    for (int st = 0; st < 4; st++) if (c->profExtract) ms[st] /= c->profExtract;
    if (c->profMatch) ms[4] /= c->profMatch;
    const int n = c->profExtract;
    c->profMax = 0;
    return n;
}

// mean host-side phase times (microseconds) of the pgorb_extract / pgorb_extract_batch calls since the last reset:
// us[0] input staging + upload issue, us[1] kernel launches + download issue, us[2] wait for the GPU, us[3] results to the caller's buffers.
// Returns the number of calls the sums cover; reset != 0 clears them (us may be NULL then).
int pgorb_profile_host(pgorb_ctx* c, double* us, int reset)
{
    if (!c) return PGORB_E_ARG;
    const int k = c->hostCalls;
    if (us) for (int i = 0; i < 4; i++) us[i] = c->hostUs[i];
    if (reset) { for (double& v : c->hostUs) v = 0; c->hostCalls = 0; }
    return k;
}

// ---- stage taps -----------------------------------------------------------------------------
static bool tap_ok(const pgorb_ctx* c, int level) { return c && c->planValid && level >= 0 && level < c->prm.nlevels; }
int pgorb_debug_level_size(const pgorb_ctx* c, int level, int* w, int* h)
{
    if (!tap_ok(c, level)) return PGORB_E_ARG;
    *w = c->plan.lvl[level].w; *h = c->plan.lvl[level].h;
    return 0;
}

int pgorb_debug_level_image(pgorb_ctx* c, int frame, int level, uint8_t* out)
{
    if (!tap_ok(c, level) || frame < 0 || frame >= c->lastFrames) return PGORB_E_ARG;
    if (level == 0 && c->lastAliased) return fail(c, PGORB_E_ARG, "level 0 aliased the caller's buffer");
    const PgLevel& V = c->plan.lvl[level];
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipDeviceSynchronize());
    PG_HIP(c, hipMemcpy2D(out, V.w, V.img + (int64_t)frame * V.fstride, V.pitch, V.w, V.h, hipMemcpyDeviceToHost));
    return 0;
}

int pgorb_debug_level_candidates(pgorb_ctx* c, int frame, int level, int32_t* x, int32_t* y,
                                 int32_t* response, int cap)
{
    if (!tap_ok(c, level) || frame < 0 || frame >= c->lastFrames) return PGORB_E_ARG;
    const PgPlan& P = c->plan;
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipDeviceSynchronize());
    // K2's per-cell slots of the level (K3 reads them in place since round 4: no dense candidate records exist any more)
    const PgLevel& V = P.lvl[level];
    const int ncells = V.nCols * V.nRows;
    std::vector<int32_t> cc(ncells);
    std::vector<uint32_t> slots((size_t)ncells * V.cellCap);
    PG_HIP(c, hipMemcpy(cc.data(), P.cellCount + (int64_t)frame * P.totalCells + V.cellBase, (size_t)ncells * 4, hipMemcpyDeviceToHost));
    PG_HIP(c, hipMemcpy(slots.data(), P.cellCand + (int64_t)frame * P.cellCandFrame + V.cellCandOff, slots.size() * 4, hipMemcpyDeviceToHost));
    int cnt = 0;
    for (int ci = 0; ci < ncells; ci++)
        for (int j = 0; j < std::min(cc[ci], V.cellCap); j++, cnt++) {
            if (cnt >= cap) continue;
            const uint32_t v = slots[(size_t)ci * V.cellCap + j];
            x[cnt] = v & 0xFFF; y[cnt] = (v >> 12) & 0xFFF; response[cnt] = v >> 24;
        }
    int32_t k3 = 0;                                            // K3's own count of the same slots must agree
    PG_HIP(c, hipMemcpy(&k3, P.candCount + frame * PG_MAXL + level, 4, hipMemcpyDeviceToHost));
    if (k3 != cnt) return fail(c, PGORB_E_OVERFLOW, "level %d: K3 counted %d candidates, the cell slots hold %d", level, k3, cnt);
    return cnt;
}

int pgorb_debug_level_keypoints(pgorb_ctx* c, int frame, int level)
{
    if (!tap_ok(c, level) || frame < 0 || frame >= c->lastFrames) return PGORB_E_ARG;
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipDeviceSynchronize());
    int32_t cnt = 0;
    PG_HIP(c, hipMemcpy(&cnt, c->plan.kpCount + frame * PG_MAXL + level, 4, hipMemcpyDeviceToHost));
    return cnt;
}

// ---- the context's shared arenas, for tests of one long-lived context (read-only; nothing in the library reads these) ------
int pgorb_debug_arena(const pgorb_ctx* c, int which, const void** ptr, int64_t* bytes)
{
    if (!c || !ptr || !bytes) return PGORB_E_ARG;
    if (which == PGORB_ARENA_PINNED) { *ptr = c->pinned; *bytes = (int64_t)c->pinnedBytes; return 0; }
    const Arena* all[] = {&c->stageA, nullptr, &c->stageSfi, &c->stageOut, &c->xdesc, &c->outBlk, &c->vocab, &c->pyr, &c->tables};
    if (which < 0 || which >= (int)(sizeof(all) / sizeof(all[0]))) return PGORB_E_ARG;
    *ptr = all[which]->p; *bytes = (int64_t)all[which]->bytes;
    return 0;
}

int pgorb_debug_host_graph(const pgorb_ctx* c, int* last_call, int* plan_epoch)
{
    if (!c || !last_call || !plan_epoch) return PGORB_E_ARG;
    *last_call = c->hg.last; *plan_epoch = c->planEpoch;
    return 0;
}

}  // extern "C"
