// stream.hip -- pgorb_stream_*: batches of frames through the extractor, the matcher and the optional front-end stage without
// blocking the host, from host memory (streamed ingest) or from device memory (device-resident form).
#include "pgorb_ctx.h"

#include <thread>

// ---- streamed ingest: frames that start in HOST memory ----------------------------------------------
// The reference's frames come from the decoder one at a time (src/io/image_sequence_reader.cc:138-208) and are
// consumed by the tracking loop (src/slam/track_image_sequence.cc:43-47).  Here the decoder writes grey frames
// straight into page-locked input slots; a slot (one batch) then flows through three HIP streams --
//   copy-in:  H2D of the slot's frames                        (PCIe, ~2.07 MB per 1080p frame)
//   compute:  K1..K6 on the slot's device frames (level 0 aliases them) + K7 of every frame against its
//             predecessor, including the last frame of the previous batch
//   copy-out: D2H of counts, keypoints, descriptors, matches into the slot's page-locked result block
// so that the upload of batch i+1 and the download of batch i-1 overlap the kernels of batch i.  Events order
// the three streams per slot; nothing blocks the host until pgorb_stream_wait.
struct pgorb_stream {
    pgorb_ctx* c = nullptr;
    int w = 0, h = 0, B = 0, depth = 0, cap = 0;               // w x h: the UPRIGHT frame the extractor sees
    // input format of the slots (pgorb_stream_create_ingest): frames exactly as decoded -- srcW x srcH pixels of `ch`
    // interleaved bytes, rotation / flips / grey conversion done on the device in front of K1 (k_ingest*, pyramid.hip)
    int srcW = 0, srcH = 0, ch = 1, rgbOrder = 1, rot = 0, vflip = 0, hflip = 0;
    bool ingest = false;                                      // false: grey, upright -> level 0 aliases the slot's device frames
    size_t inBytes = 0;                                       // bytes per input frame
    bool dead = false;                                        // a submit failed half way: the stream only accepts destroy
    hipStream_t sIn = nullptr, sRun = nullptr, sOut = nullptr;
    // Device-resident form (pgorb_stream_create_device, round 5): frames come from the caller's device memory, results stay
    // on the device, and consecutive batches run on `lanes` independent extractor working sets (lane 0 = the context itself,
    // the others private sibling contexts with the same parameters and options), each on its own HIP stream -- two batches
    // in flight let K1 (HBM), K2 / K4-6 (VALU issue), K3 (latency) and K7 (matrix pipe) of neighbouring batches share the chip.
    // Slot k runs on lane k % lanes.  What crosses batches -- the previous batch's last frame for the first match, the
    // front-end stage's state -- is one short section per batch; the sections run in submission order on a stream of their
    // own (sChain), each behind its batch's K1..K6, so the lanes never wait for each other: they drift apart and kernels of
    // DIFFERENT kinds end up side by side (a first build queued the section at the end of the lane's own stream, chained by
    // an event: the lanes then ran in lockstep, K1 beside K1 and K2 beside K2, and gained nothing -- 98.1 k against 98.3 k).
    bool device = false;
    std::vector<pgorb_ctx*> lane;          // [0] = c
    std::vector<hipStream_t> sLane;        // [0] = sRun
    hipStream_t sChain = nullptr;          // the sections that cross batches, in submission order (several lanes: a stream of its own)
    int32_t* hStatus = nullptr;            // pinned, one word per slot (device form: the batch's status word)
    struct Slot {
        uint8_t* hIn = nullptr;            // pinned [B][srcH][srcW][ch]
        uint8_t* dIn = nullptr;            // device copy of it
        uint8_t* dOut = nullptr;           // device result block (layout below)
        uint8_t* hOut = nullptr;           // pinned copy of it
        hipEvent_t evIn = nullptr, evRun = nullptr, evOut = nullptr, evExt = nullptr;   // evExt: K1..K6 of the slot's batch done (device form)
        int frames = 0; bool busy = false;
    };
    std::vector<Slot> slot;
    // result block: n[B+1] (index 0 = the previous batch's last frame) | kps[B][cap] | desc[B+1][cap][32] |
    // best_idx[B][cap] | best[B][cap] | second[B][cap]
    size_t offN = 0, offK = 0, offD = 0, offI = 0, offB1 = 0, offB2 = 0, outBytes = 0;
    int32_t *dPq = nullptr, *dPt = nullptr;                // pairs (f, f-1), f = 1..B, in desc[] indexing
    uint8_t* dPrevDesc = nullptr; int32_t* dPrevN = nullptr; pgorb_keypoint* dPrevKps = nullptr;
    bool havePrev = false;
    // optional front-end stage (pgorb_stream_frontend): + matches12[B][cap] | nmatches[B] | word[B][cap] | weight[B][cap] | node[B][cap]
    bool fe = false; int feWindow = 100, feCheckOri = 1, feLevelsUp = -1; float feRatio = 0.9f, feBounds[4] = {0, 0, 0, 0};
    size_t offM12 = 0, offNM = 0, offW = 0, offWt = 0, offNd = 0;
    int32_t *dGridStart = nullptr, *dGridIdx = nullptr; float* dPrevMatched = nullptr;     // device scratch, [B+1] frames
};

// result-block layout for the stream's current settings (kps and desc hold B+1 frames: index 0 = the previous batch's last frame)
static void stream_layout(pgorb_stream* s)
{
    const size_t cap = (size_t)s->cap, B = (size_t)s->B;
    auto al = [](size_t v) { return (v + 255) / 256 * 256; };
    s->offN = 0; s->offK = al((B + 1) * 4); s->offD = s->offK + al((B + 1) * cap * sizeof(pgorb_keypoint));
    s->offI = s->offD + al((B + 1) * cap * 32); s->offB1 = s->offI + al(B * cap * 4);
    s->offB2 = s->offB1 + al(B * cap * 2); s->outBytes = s->offB2 + al(B * cap * 2);
    if (s->fe) {
        s->offM12 = s->outBytes; s->offNM = s->offM12 + al(B * cap * 4); s->outBytes = s->offNM + al(B * 4);
        if (s->feLevelsUp >= 0) {
            s->offWt = s->outBytes; s->offW = s->offWt + al(B * cap * 8); s->offNd = s->offW + al(B * cap * 4);
            s->outBytes = s->offNd + al(B * cap * 4);
        }
    }                                                        // (+ the status word behind it)
}

// what both stream forms allocate: the result-block layout, every slot's device result block and its upload / run events, the
// pairs (f, f-1), the previous batch's last frame, and the matcher scratch of a batch
static bool stream_alloc_common(pgorb_stream* s)
{
    pgorb_ctx* c = s->c;
    const size_t cap = (size_t)s->cap, B = (size_t)s->B;
    stream_layout(s);
    s->slot.resize(s->depth);
    bool ok = true;
    for (auto& sl : s->slot) {
        ok = ok && hipMalloc((void**)&sl.dOut, s->outBytes + 256) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&sl.evIn, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&sl.evRun, hipEventDisableTiming) == hipSuccess;
    }
    std::vector<int32_t> pq(B), pt(B);
    for (int f = 0; f < s->B; f++) { pq[f] = f + 1; pt[f] = f; }
    ok = ok && hipMalloc((void**)&s->dPq, B * 4) == hipSuccess && hipMalloc((void**)&s->dPt, B * 4) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->dPrevDesc, cap * 32) == hipSuccess && hipMalloc((void**)&s->dPrevN, 4) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->dPrevKps, cap * sizeof(pgorb_keypoint)) == hipSuccess;
    ok = ok && hipMemcpy(s->dPq, pq.data(), B * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(s->dPt, pt.data(), B * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && ensure(c, c->xdesc, pg_match_scratch_bytes(c->mx, s->cap, s->B) + 16) == 0;
    return ok;
}

// what a wait returns for a collected slot: the batch's device status `st` if it is set, else the result pointers into the slot's
// host (pgorb_stream_wait) or device (pgorb_stream_wait_device) result block
static int stream_results(const pgorb_stream* s, const pgorb_stream::Slot& sl, const uint8_t* base, int32_t st, const int32_t** n,
                          const pgorb_keypoint** kps, const uint8_t** desc, const int32_t** best_idx, const uint16_t** best,
                          const uint16_t** second, int* cap)
{
    if (st) return fail(s->c, st, "device reported status %d", st);
    if (n) *n = (const int32_t*)(base + s->offN) + 1;
    if (kps) *kps = (const pgorb_keypoint*)(base + s->offK) + s->cap;
    if (desc) *desc = base + s->offD + (size_t)s->cap * 32;
    if (best_idx) *best_idx = (const int32_t*)(base + s->offI);
    if (best) *best = (const uint16_t*)(base + s->offB1);
    if (second) *second = (const uint16_t*)(base + s->offB2);
    if (cap) *cap = s->cap;
    return sl.frames;
}

// wait for everything queued on the stream object's HIP streams (sRun is sLane[0], and sChain too with one lane)
static void stream_drain(pgorb_stream* s)
{
    for (hipStream_t q : {s->sIn, s->sRun, s->sOut, s->sChain}) if (q) (void)hipStreamSynchronize(q);
    for (hipStream_t q : s->sLane) if (q) (void)hipStreamSynchronize(q);
}

// the buffers that pgorb_stream_frontend replaces (every slot's result blocks) or adds (the stage's device scratch)
static void stream_free_results(pgorb_stream* s)
{
    for (auto& sl : s->slot) {
        if (sl.dOut) (void)hipFree(sl.dOut);
        if (sl.hOut) (void)hipHostFree(sl.hOut);
    }
}
static void stream_free_grid(pgorb_stream* s)
{
    for (void* p : {(void*)s->dGridStart, (void*)s->dGridIdx, (void*)s->dPrevMatched}) if (p) (void)hipFree(p);
}

static int stream_submit_queue(pgorb_stream* s, pgorb_stream::Slot& sl, int nframes, int slotIndex, const uint8_t* d_frames,
                               int stride, int64_t frame_stride, hipStream_t caller)
{
    pgorb_ctx* c = s->c;                                       // errors, the vocabulary and the matchers' scratch live here
    const int laneIx = s->device ? slotIndex % (int)s->lane.size() : 0;
    pgorb_ctx* lc = s->lane[laneIx];                           // the extractor working set this batch runs on
    hipStream_t sr = s->sLane[laneIx];
    int rc;
    const size_t fbytes = s->inBytes, cap = (size_t)s->cap;
    if (!s->device) {
        // copy-in: after the kernels of this slot's previous batch have read its device frames
        PG_HIP(c, hipStreamWaitEvent(s->sIn, sl.evRun, 0));
        PG_HIP(c, hipMemcpyAsync(sl.dIn, sl.hIn, fbytes * nframes, hipMemcpyHostToDevice, s->sIn));
        PG_HIP(c, hipEventRecord(sl.evIn, s->sIn));
        // compute: after the upload, and after the previous download of this slot's result block
        PG_HIP(c, hipStreamWaitEvent(sr, sl.evIn, 0));
        PG_HIP(c, hipStreamWaitEvent(sr, sl.evOut, 0));
    } else {
        // the caller's frames are ready where the caller's stream stands now; the slot's result block is free once the
        // section of the batch that used it last is done (a never-recorded event does not wait)
        PG_HIP(c, hipEventRecord(sl.evIn, caller));
        PG_HIP(c, hipStreamWaitEvent(sr, sl.evIn, 0));
        PG_HIP(c, hipStreamWaitEvent(sr, sl.evRun, 0));
        // (holding a batch back until the previous lane's batch is past its pyramid or its K2 measured slower on an MI355X: 101.1 k /
        // 99.0 k frames/s against 101.3 k at 1080p / 2000, batch 128 -- the hardware interleaves the lanes' kernels at workgroup
        // granularity whatever the start offsets; tools/experiments/r5_lanes.py, profiles/r05_lanes.txt)
    }
    int32_t* dN = (int32_t*)(sl.dOut + s->offN);
    pgorb_keypoint* dK = (pgorb_keypoint*)(sl.dOut + s->offK);
    uint8_t* dD = sl.dOut + s->offD;
    // ---- extraction: K1..K6 of this batch alone (nothing here looks at another batch) ----
    if (s->device) {
        rc = run_batch(lc, d_frames, false, nframes, s->w, s->h, stride, frame_stride, dK + cap, dD + cap * 32, s->cap, dN + 1, sr);
        if (rc && lc != c) c->err = lc->err;
    } else if (s->ingest) {
        // frames as decoded: rotation / flips / cvtColor on the device into level 0 (image_sequence_reader.cc:53-58,186-205;
        // Tracking.cc:247-260), then the extractor on the upright grey planes
        pg_launch_ingest(c->plan, sl.dIn, s->srcW * s->ch, (int64_t)fbytes, s->srcW, s->srcH, s->ch, s->rgbOrder, s->rot,
                         s->vflip != 0, s->hflip != 0, nframes, sr);
        rc = run_batch(c, nullptr, true, nframes, s->w, s->h, s->w, 0, dK + cap, dD + cap * 32, s->cap, dN + 1, sr);
    } else {
        rc = run_batch(c, sl.dIn, false, nframes, s->w, s->h, s->w, (int64_t)fbytes, dK + cap, dD + cap * 32, s->cap, dN + 1, sr);
    }
    if (rc) return rc;
    // the batch's device status word travels inside the result block (the lane's next batch resets the word)
    PG_HIP(c, hipMemcpyAsync(sl.dOut + s->outBytes, lc->plan.status, 4, hipMemcpyDeviceToDevice, sr));
    if (s->device) PG_HIP(c, hipMemcpyAsync(s->hStatus + slotIndex, lc->plan.status, 4, hipMemcpyDeviceToHost, sr));
    // ---- the section that crosses batches: in submission order on sChain, behind this batch's K1..K6 ----
    if (s->sChain != sr) {
        PG_HIP(c, hipEventRecord(sl.evExt, sr));
        PG_HIP(c, hipStreamWaitEvent(s->sChain, sl.evExt, 0));
        sr = s->sChain;
    }
    if (s->havePrev) {
        PG_HIP(c, hipMemcpyAsync(dD, s->dPrevDesc, cap * 32, hipMemcpyDeviceToDevice, sr));
        PG_HIP(c, hipMemcpyAsync(dN, s->dPrevN, 4, hipMemcpyDeviceToDevice, sr));
        if (s->fe) PG_HIP(c, hipMemcpyAsync(dK, s->dPrevKps, cap * sizeof(pgorb_keypoint), hipMemcpyDeviceToDevice, sr));
    } else {
        PG_HIP(c, hipMemsetAsync(dN, 0, 4, sr));
    }
    // the slab form (match_mode 0) may have been selected after the stream was created: size its arena for THIS launch
    // (ensure() only ever grows; hipFree of the old arena waits for the work that still uses it)
    if ((rc = ensure(c, c->xdesc, pg_match_scratch_bytes(c->mx, s->cap, nframes) + 16))) return rc;
    pg_launch_match_batch(c->mx, dD, dN, s->cap, s->dPq, s->dPt, nframes, (uint8_t*)c->xdesc.p, (int32_t*)(sl.dOut + s->offI),
                          (uint16_t*)(sl.dOut + s->offB1), (uint16_t*)(sl.dOut + s->offB2), sr);
    if (s->fe) {
        // what the tracking thread does with a fresh Frame, for the whole batch: the 64x48 grid of every frame
        // (Frame.cc:234-249), SearchForInitialization(previous, current) with vbPrevMatched = the previous frame's
        // keypoints (Tracking.cc:583-597), ORBVocabulary::transform of every descriptor (Frame.cc:399-406)
        const float* b = s->feBounds;
        if ((rc = pgorb_frame_grid_batch_device(c, dK + cap, dN + 1, nframes, s->cap, b[0], b[1], b[2], b[3],
                                                s->dGridStart + (PGORB_GRID_CELLS + 1), s->dGridIdx + cap, sr))) return rc;
        pg_launch_prev_matched_init(dK, (int64_t)nframes * cap, s->dPrevMatched, sr);
        if ((rc = pgorb_search_for_initialization_batch_device(c, dK, dD, dN, s->cap, s->dGridStart, s->dGridIdx, s->dPt, s->dPq, nframes,
                                                               b[0], b[1], b[2], b[3], s->dPrevMatched, (int32_t*)(sl.dOut + s->offM12),
                                                               (int32_t*)(sl.dOut + s->offNM), s->feWindow, s->feRatio, s->feCheckOri, sr))) return rc;
        if (s->feLevelsUp >= 0 &&
            (rc = pgorb_bow_transform_device(c, dD + cap * 32, nframes * s->cap, s->feLevelsUp, (uint32_t*)(sl.dOut + s->offW),
                                             (double*)(sl.dOut + s->offWt), (uint32_t*)(sl.dOut + s->offNd), sr))) return rc;
        PG_HIP(c, hipMemcpyAsync(s->dPrevKps, dK + (size_t)nframes * cap, cap * sizeof(pgorb_keypoint), hipMemcpyDeviceToDevice, sr));
    }
    PG_HIP(c, hipMemcpyAsync(s->dPrevDesc, dD + (size_t)nframes * cap * 32, cap * 32, hipMemcpyDeviceToDevice, sr));
    PG_HIP(c, hipMemcpyAsync(s->dPrevN, dN + nframes, 4, hipMemcpyDeviceToDevice, sr));
    PG_HIP(c, hipEventRecord(sl.evRun, sr));
    s->havePrev = true;
    if (!s->device) {
        // copy-out
        PG_HIP(c, hipStreamWaitEvent(s->sOut, sl.evRun, 0));
        PG_HIP(c, hipMemcpyAsync(sl.hOut, sl.dOut, s->outBytes + 4, hipMemcpyDeviceToHost, s->sOut));
        PG_HIP(c, hipEventRecord(sl.evOut, s->sOut));
    }
    PG_HIP(c, hipGetLastError());
    return 0;
}

// What both submit calls end with: the plan of the slot's lane, the batch queued, the slot marked busy.  A batch that fails half way
// may be queued in part with no event recorded for the slot: drain, so that nothing still writes into its buffers, and retire the stream.
static int stream_submit(pgorb_stream* s, int slot, int nframes, const uint8_t* d_frames = nullptr, int stride = 0,
                         int64_t frame_stride = 0, hipStream_t caller = nullptr)
{
    pgorb_ctx *c = s->c, *lc = s->lane[slot % (int)s->lane.size()];
    pgorb_stream::Slot& sl = s->slot[slot];
    int rc = make_plan(lc, s->w, s->h, nframes);
    if (rc) { if (lc != c) c->err = lc->err; return rc; }
    if ((rc = stream_submit_queue(s, sl, nframes, slot, d_frames, stride, frame_stride, caller))) {
        stream_drain(s);
        s->dead = true;
        return rc;
    }
    sl.frames = nframes; sl.busy = true;
    return 0;
}

extern "C" {

int pgorb_stream_create(pgorb_ctx* c, int w, int h, int batch, int depth, pgorb_stream** out)
{
    return pgorb_stream_create_ingest(c, w, h, 1, 1, 0, 0, 0, batch, depth, out);
}

int pgorb_stream_create_ingest(pgorb_ctx* c, int src_w, int src_h, int channels, int rgb_order, int rotate_degrees,
                               int vertical_flip, int horizontal_flip, int batch, int depth, pgorb_stream** out)
{
    if (!c || !out) return PGORB_E_ARG;
    *out = nullptr;
    if (batch < 1 || batch > c->prm.max_batch || depth < 2 || depth > 8 || src_w < 1 || src_h < 1)
        return fail(c, PGORB_E_ARG, "pgorb_stream_create: batch 1..max_batch, depth 2..8");
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(c, PGORB_E_ARG, "pgorb_stream_create_ingest: channels must be 1, 3 or 4");
    int w, h, rc;
    if ((rc = upright_size(c, rotate_degrees, src_w, src_h, &w, &h)) || (rc = make_plan(c, w, h, batch))) return rc;
    pgorb_stream* s = new pgorb_stream();
    s->c = c; s->w = w; s->h = h; s->B = batch; s->depth = depth; s->cap = c->plan.selTotal;
    s->srcW = src_w; s->srcH = src_h; s->ch = channels; s->rgbOrder = rgb_order ? 1 : 0; s->rot = rotate_degrees / 90;
    s->vflip = vertical_flip ? 1 : 0; s->hflip = horizontal_flip ? 1 : 0;
    s->ingest = channels != 1 || s->rot || s->vflip || s->hflip;
    s->inBytes = (size_t)src_w * src_h * channels;
    const size_t B = (size_t)batch;
    bool ok = stream_alloc_common(s);
    ok = ok && hipStreamCreateWithFlags(&s->sIn, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&s->sRun, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&s->sOut, hipStreamNonBlocking) == hipSuccess;
    {
        // the page-locked input slots are the expensive part of a stream (0.3 ms per MB: 128 MB per slot of 64 1080p frames):
        // one thread per slot page-locks its buffers (round 4: the CLI's start-up; a third of the time with three slots)
        std::vector<int> okSlot(depth, 1);
        std::vector<std::thread> th;
        const int dev = c->prm.device;
        auto allocSlot = [&](int k) {
            pgorb_stream::Slot& sl = s->slot[k];
            bool o = hipSetDevice(dev) == hipSuccess;
            o = o && hipHostMalloc((void**)&sl.hIn, B * s->inBytes, hipHostMallocDefault) == hipSuccess;
            o = o && hipHostMalloc((void**)&sl.hOut, s->outBytes + 256, hipHostMallocDefault) == hipSuccess;
            okSlot[k] = o ? 1 : 0;
        };
        for (int k = 1; k < depth; k++) th.emplace_back(allocSlot, k);
        allocSlot(0);
        for (auto& t : th) t.join();
        for (int k = 0; k < depth; k++) ok = ok && okSlot[k];
    }
    for (auto& sl : s->slot) {
        ok = ok && hipMalloc((void**)&sl.dIn, B * s->inBytes + 256) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&sl.evOut, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) { pgorb_stream_destroy(s); return fail(c, PGORB_E_HIP, "pgorb_stream_create: allocation failed"); }
    s->lane.assign(1, c); s->sLane.assign(1, s->sRun); s->sChain = s->sRun;
    c->streams.push_back(s);
    *out = s;
    return 0;
}

void pgorb_stream_destroy(pgorb_stream* s)
{
    if (!s) return;
    (void)hipSetDevice(s->c->prm.device);
    auto& live = s->c->streams;
    live.erase(std::remove(live.begin(), live.end(), s), live.end());
    stream_drain(s);
    for (size_t l = 1; l < s->sLane.size(); l++) if (s->sLane[l]) (void)hipStreamDestroy(s->sLane[l]);
    for (size_t l = 1; l < s->lane.size(); l++) pgorb_destroy(s->lane[l]);      // the private sibling contexts
    if (s->sChain && s->lane.size() > 1) (void)hipStreamDestroy(s->sChain);
    if (s->hStatus) (void)hipHostFree(s->hStatus);
    stream_free_results(s);
    stream_free_grid(s);
    for (auto& sl : s->slot) {
        if (sl.hIn) (void)hipHostFree(sl.hIn);
        if (sl.dIn) (void)hipFree(sl.dIn);
        for (hipEvent_t e : {sl.evIn, sl.evRun, sl.evOut, sl.evExt}) if (e) (void)hipEventDestroy(e);
    }
    for (void* p : {(void*)s->dPq, (void*)s->dPt, (void*)s->dPrevDesc, (void*)s->dPrevN, (void*)s->dPrevKps}) if (p) (void)hipFree(p);
    for (hipStream_t q : {s->sIn, s->sRun, s->sOut}) if (q) (void)hipStreamDestroy(q);
    delete s;
}

uint8_t* pgorb_stream_input(pgorb_stream* s, int slot)
{
    return (s && slot >= 0 && slot < s->depth) ? s->slot[slot].hIn : nullptr;
}

int pgorb_stream_reset(pgorb_stream* s)                  // a new ride: the next batch has no predecessor frame
{
    if (!s) return PGORB_E_ARG;
    s->havePrev = false;
    return 0;
}

int pgorb_stream_submit(pgorb_stream* s, int slot, int nframes)
{
    if (!s || slot < 0 || slot >= s->depth) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    if (nframes < 1 || nframes > s->B) return fail(c, PGORB_E_ARG, "pgorb_stream_submit: 1..batch frames");
    if (s->dead) return fail(c, PGORB_E_HIP, "pgorb_stream_submit: an earlier submit failed half way; destroy the stream");
    if (s->device) return fail(c, PGORB_E_ARG, "pgorb_stream_submit: a device-resident stream takes pgorb_stream_submit_device");
    pgorb_stream::Slot& sl = s->slot[slot];
    if (sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_submit: slot %d not collected with pgorb_stream_wait", slot);
    return stream_submit(s, slot, nframes);
}

int pgorb_stream_wait(pgorb_stream* s, int slot, const int32_t** n, const pgorb_keypoint** kps, const uint8_t** desc,
                      const int32_t** best_idx, const uint16_t** best, const uint16_t** second, int* cap)
{
    if (!s || slot < 0 || slot >= s->depth) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    pgorb_stream::Slot& sl = s->slot[slot];
    if (s->device) return fail(c, PGORB_E_ARG, "pgorb_stream_wait: a device-resident stream takes pgorb_stream_wait_device");
    if (!sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_wait: slot %d has no batch in flight", slot);
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipEventSynchronize(sl.evOut));
    sl.busy = false;
    const int32_t st = *(const int32_t*)(sl.hOut + s->outBytes);      // the batch's device status word
    return stream_results(s, sl, sl.hOut, st, n, kps, desc, best_idx, best, second, cap);
}

// The device-resident form: `lanes` extractor working sets behind one stream object (include/pgorb.h), sibling contexts with
// "the same parameters and options": copy_tunables at lane creation, and pgorb_set_option forwards later changes here.
void pg_forward_option_to_lanes(pgorb_ctx* c, const char* key, int value)
{
    for (pgorb_stream* st : c->streams)
        for (size_t l = 1; l < st->lane.size(); l++)
            if (st->lane[l] && st->lane[l] != c) (void)pgorb_set_option(st->lane[l], key, value);
}

int pgorb_stream_create_device(pgorb_ctx* c, int w, int h, int batch, int depth, int lanes, pgorb_stream** out)
{
    if (!c || !out) return PGORB_E_ARG;
    *out = nullptr;
    if (batch < 1 || batch > c->prm.max_batch || depth < 2 || depth > 8 || lanes < 1 || lanes > depth || w < 1 || h < 1)
        return fail(c, PGORB_E_ARG, "pgorb_stream_create_device: batch 1..max_batch, depth 2..8, lanes 1..depth");
    if (int rc = make_plan(c, w, h, batch)) return rc;
    pgorb_stream* s = new pgorb_stream();
    s->c = c; s->w = w; s->h = h; s->B = batch; s->depth = depth; s->cap = c->plan.selTotal;
    s->srcW = w; s->srcH = h; s->ch = 1; s->device = true;
    s->inBytes = (size_t)w * h;
    s->lane.assign(1, c);
    bool ok = hipStreamCreateWithFlags(&s->sRun, hipStreamNonBlocking) == hipSuccess;
    s->sLane.assign(1, s->sRun);
    for (int l = 1; l < lanes && ok; l++) {
        // a sibling context: the same extractor (parameters, options), its own pyramid / candidate / selection arenas and plan
        pgorb_ctx* lc = nullptr;
        hipStream_t ls = nullptr;
        ok = pgorb_create(&c->prm, &lc) == PGORB_OK;
        if (ok) {
            copy_tunables(lc, c);
            s->lane.push_back(lc);
            ok = make_plan(lc, w, h, batch) == 0 && hipStreamCreateWithFlags(&ls, hipStreamNonBlocking) == hipSuccess;
            s->sLane.push_back(ls);
        }
    }
    ok = ok && hipHostMalloc((void**)&s->hStatus, 64 * sizeof(int32_t), hipHostMallocDefault) == hipSuccess;
    if (lanes > 1) ok = ok && hipStreamCreateWithFlags(&s->sChain, hipStreamNonBlocking) == hipSuccess;
    else s->sChain = s->sRun;
    ok = ok && stream_alloc_common(s);
    for (auto& sl : s->slot) ok = ok && hipEventCreateWithFlags(&sl.evExt, hipEventDisableTiming) == hipSuccess;
    if (!ok) { pgorb_stream_destroy(s); return fail(c, PGORB_E_HIP, "pgorb_stream_create_device: allocation failed"); }
    c->streams.push_back(s);
    *out = s;
    return 0;
}

int pgorb_stream_submit_device(pgorb_stream* s, int slot, const uint8_t* d_frames, int nframes, int stride, int64_t frame_stride,
                               void* hip_stream)
{
    if (!s || slot < 0 || slot >= s->depth) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    if (!s->device) return fail(c, PGORB_E_ARG, "pgorb_stream_submit_device: the stream was created for host frames");
    if (nframes < 1 || nframes > s->B || !d_frames || stride < s->w) return fail(c, PGORB_E_ARG, "pgorb_stream_submit_device: 1..batch frames, stride >= width");
    if (s->dead) return fail(c, PGORB_E_HIP, "pgorb_stream_submit_device: an earlier submit failed half way; destroy the stream");
    pgorb_stream::Slot& sl = s->slot[slot];
    if (sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_submit_device: slot %d not collected with pgorb_stream_wait_device", slot);
    return stream_submit(s, slot, nframes, d_frames, stride, frame_stride, (hipStream_t)hip_stream);
}

// Device-resident form: the slot's batch is complete (host blocks on the batch's event, or -- hip_stream != NULL with
// wait_on_host == 0 -- that stream is made to wait for it and the call returns at once); DEVICE pointers into the slot's
// result block, valid until the slot is submitted again.
int pgorb_stream_wait_device(pgorb_stream* s, int slot, int wait_on_host, void* hip_stream, const int32_t** d_n, const pgorb_keypoint** d_kps,
                             const uint8_t** d_desc, const int32_t** d_best_idx, const uint16_t** d_best, const uint16_t** d_second, int* cap)
{
    if (!s || slot < 0 || slot >= s->depth) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    if (!s->device) return fail(c, PGORB_E_ARG, "pgorb_stream_wait_device: the stream was created for host frames");
    pgorb_stream::Slot& sl = s->slot[slot];
    if (!sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_wait_device: slot %d has no batch in flight", slot);
    PG_HIP(c, hipSetDevice(c->prm.device));
    int32_t st = 0;
    if (wait_on_host) {                                       // (hip_stream == NULL is the legacy null stream, as in pgorb_stream_submit_device)
        PG_HIP(c, hipEventSynchronize(sl.evRun));
        st = s->hStatus[slot];
    } else {
        PG_HIP(c, hipStreamWaitEvent((hipStream_t)hip_stream, sl.evRun, 0));        // (the status word: pgorb_check_async of the caller's choice)
    }
    sl.busy = false;
    return stream_results(s, sl, sl.dOut, st, d_n, d_kps, d_desc, d_best_idx, d_best, d_second, cap);
}

int pgorb_stream_lanes(const pgorb_stream* s) { return s ? (int)s->lane.size() : PGORB_E_ARG; }

int pgorb_stream_frontend(pgorb_stream* s, float min_x, float max_x, float min_y, float max_y, int window_size, float nnratio,
                          int check_orientation, int bow_levelsup)
{
    if (!s) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    if (!(max_x > min_x) || !(max_y > min_y) || window_size < 0) return fail(c, PGORB_E_ARG, "pgorb_stream_frontend: bounds / window");
    for (auto& sl : s->slot) if (sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_frontend: a batch is in flight");
    if (s->cap > 16000) return fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (bow_levelsup >= 0) {
        const uint8_t* blob; int k, L, nn;
        int rc = pg_ctx_vocab_get(c, &blob, &k, &L, &nn);     // "no vocabulary resident" is reported here, not at the first submit
        if (rc) return rc;
    }
    PG_HIP(c, hipSetDevice(c->prm.device));
    PG_HIP(c, hipDeviceSynchronize());
    // new result blocks first, on a copy; the stream's settings and buffers change only when every allocation succeeded
    pgorb_stream t = *s;
    t.fe = true; t.feLevelsUp = bow_levelsup;
    stream_layout(&t);
    const size_t cap = (size_t)s->cap, B = (size_t)s->B;
    const bool newGrid = !s->dGridStart;
    bool ok = true;
    for (auto& sl : t.slot) {
        sl.dOut = sl.hOut = nullptr;
        ok = ok && hipMalloc((void**)&sl.dOut, t.outBytes + 256) == hipSuccess;
        ok = ok && (s->device || hipHostMalloc((void**)&sl.hOut, t.outBytes + 256, hipHostMallocDefault) == hipSuccess);
    }
    if (newGrid) {
        ok = ok && hipMalloc((void**)&t.dGridStart, (B + 1) * (PGORB_GRID_CELLS + 1) * 4) == hipSuccess;
        ok = ok && hipMalloc((void**)&t.dGridIdx, (B + 1) * cap * 4) == hipSuccess;
        ok = ok && hipMalloc((void**)&t.dPrevMatched, B * cap * 8) == hipSuccess;
    }
    if (!ok) {
        stream_free_results(&t);
        if (newGrid) stream_free_grid(&t);
        return fail(c, PGORB_E_HIP, "pgorb_stream_frontend: allocation failed (the stream is unchanged)");
    }
    stream_free_results(s);
    for (size_t i = 0; i < s->slot.size(); i++) { s->slot[i].dOut = t.slot[i].dOut; s->slot[i].hOut = t.slot[i].hOut; }
    s->dGridStart = t.dGridStart; s->dGridIdx = t.dGridIdx; s->dPrevMatched = t.dPrevMatched;
    s->fe = true; s->feWindow = window_size; s->feRatio = nnratio; s->feCheckOri = check_orientation ? 1 : 0; s->feLevelsUp = bow_levelsup;
    s->feBounds[0] = min_x; s->feBounds[1] = max_x; s->feBounds[2] = min_y; s->feBounds[3] = max_y;
    stream_layout(s);
    s->havePrev = false;
    return 0;
}

int pgorb_stream_frontend_results(pgorb_stream* s, int slot, const int32_t** matches12, const int32_t** nmatches,
                                  const uint32_t** word, const double** weight, const uint32_t** node)
{
    if (!s || slot < 0 || slot >= s->depth) return PGORB_E_ARG;
    pgorb_ctx* c = s->c;
    pgorb_stream::Slot& sl = s->slot[slot];
    if (!s->fe) return fail(c, PGORB_E_ARG, "pgorb_stream_frontend_results: the front-end stage is not enabled");
    if (sl.busy) return fail(c, PGORB_E_ARG, "pgorb_stream_frontend_results: collect slot %d with pgorb_stream_wait first", slot);
    const uint8_t* base = s->device ? sl.dOut : sl.hOut;      // (a device-resident stream hands out DEVICE pointers here as well)
    if (matches12) *matches12 = (const int32_t*)(base + s->offM12);
    if (nmatches) *nmatches = (const int32_t*)(base + s->offNM);
    const bool bow = s->feLevelsUp >= 0;
    if (word) *word = bow ? (const uint32_t*)(base + s->offW) : nullptr;
    if (weight) *weight = bow ? (const double*)(base + s->offWt) : nullptr;
    if (node) *node = bow ? (const uint32_t*)(base + s->offNd) : nullptr;
    return 0;
}

}  // extern "C"
