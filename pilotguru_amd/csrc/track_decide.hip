// track_decide.hip -- the decisions of the tracking thread between its numeric steps, on resident arrays, on gfx950.
//
// Restates (thirdparty/orb-slam2):
//   Tracking::CheckReplacedInLastFrame                   src/Tracking.cc:735-745
//   SearchLocalPoints' two IncreaseVisible               :1148, :1168
//   the discard loops' mnLastFrameSeen                   :781, :904
//   bOK of TrackReferenceKeyFrame / TrackWithMotionModel / TrackLocalMap   :760, :789 / :879-886, :918 / :932-964
//   Track()'s tail: clean VO matches, NeedNewKeyFrame, CreateNewKeyFrame, the outlier discard   :445-476, :968-1052, :1054-1132
//   KeyFrame::TrackedMapPoints, ComputeSceneMedianDepth  src/KeyFrame.cc:353-378, :736-766
//   CreateInitialMapMonocular's unit median depth        src/Tracking.cc:684-709
// under the readings of DESIGN.md section 4 (the decision rows).
//   k_td_replaced, k_td_visible, k_td_mark, k_td_seen   a thread per slot or query
//   k_td_decide, k_td_finish    a workgroup per tracker: counts are wave reductions and one LDS step, the decision is one lane's,
//                               the rows are copied by all lanes
//   k_td_median                 a workgroup per list entry: order-preserving uint32 keys in LDS, an exact radix select in four 8-bit
//                               histogram passes (a histogram per wave, so that equal depths contend inside one wave only)
//   k_td_scale_head, k_td_scale_count, k_td_scale_points   the initial map's scale: the median in d_info, slot counts in scratch
// Integer atomics only count; no floating-point atomic.
#include "loop_pose.h"
#include <algorithm>
#include <set>
#include <string>
#include <vector>

#define TD_T 256
#define TD_W (TD_T / 64)
#define TD_SEEN_MAX_POINTS 1048576

static_assert(sizeof(pgorb_track_counters) == 48, "record layout");

__device__ __forceinline__ bool td_in(int p, int n) { return p >= 0 && p < n; }

// the frame of tracker t and its slot count, clamped to the row; a frame out of range has no slots
__device__ __forceinline__ int td_frame(const int32_t* n, const int32_t* frame, int t, int nframes, int cap, int& f)
{
    f = frame ? frame[t] : t;
    return td_in(f, nframes) ? min(max(n[f], 0), cap) : 0;
}

// the sum of v over the workgroup, in every lane; sh [TD_W]
__device__ __forceinline__ int td_block_sum(int v, int* sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < TD_W; w++) s += sh[w];
    return s;
}

// the table's observation lists, masked: a dead entry, or one that names nothing of the batch, does not exist
struct TdObs { int npoints; const uint8_t* bad; const int32_t* start; const int32_t* frame; int nobs; const uint8_t* live; int nframes; };

// Observations() >= minObs of point p (in range)
__device__ __forceinline__ bool td_observed(const TdObs& O, int p, int minObs)
{
    const int s = O.start[p], e = O.start[p + 1];
    if (s < 0 || e > O.nobs) return false;
    int c = 0;
    for (int j = s; j < e && c < minObs; j++) c += (!O.live || O.live[j]) && td_in(O.frame[j], O.nframes);
    return c >= minObs;
}

// KeyFrame::TrackedMapPoints(minObs) of one row, this lane's share (KeyFrame.cc:353-378; minObs > 0 in both callers)
__device__ __forceinline__ int td_tracked(const TdObs& O, const int32_t* row, int n, int minObs)
{
    int c = 0;
    for (int i = threadIdx.x; i < n; i += TD_T) {
        const int p = row[i];
        if (td_in(p, O.npoints) && !(O.bad && O.bad[p]) && td_observed(O, p, minObs)) c++;
    }
    return c;
}

// mnId < a + b and mnId >= a + b of Tracking.cc:958, :980, :1020, :1022: the sum of an unsigned int and an int is formed in 32-bit
// unsigned arithmetic and wraps, then it is widened to mnId's unsigned long
__device__ __forceinline__ uint64_t td_sum(uint32_t a, int32_t b) { return (uint64_t)(uint32_t)(a + (uint32_t)b); }

__global__ __launch_bounds__(TD_T) void k_td_replaced(int cap, int nframes, const int32_t* n, const int32_t* frame, int32_t* last, int npoints,
                                                     const int32_t* replaced)
{
    const int t = blockIdx.y, i = blockIdx.x * TD_T + threadIdx.x;
    int f;
    if (i >= td_frame(n, frame, t, nframes, cap, f)) return;
    const int p = last[(int64_t)t * cap + i];
    if (!td_in(p, npoints)) return;
    const int r = replaced[p];                                                                  // GetReplaced(): ONE step (:739-741)
    if (r >= 0) last[(int64_t)t * cap + i] = r;
}

__global__ __launch_bounds__(TD_T) void k_td_visible(int cap, int nframes, const int32_t* n, const int32_t* frame, const uint8_t* run,
                                                    const int32_t* slots, int qcap, const int32_t* nq, const int32_t* queries,
                                                    const uint8_t* inView, int npoints, int32_t* visible)
{
    const int t = blockIdx.y, i = blockIdx.x * TD_T + threadIdx.x;
    if (run && !run[t]) return;
    int f;
    if (i < td_frame(n, frame, t, nframes, cap, f)) {                                           // :1148
        const int p = slots[(int64_t)t * cap + i];
        if (td_in(p, npoints)) atomicAdd(&visible[p], 1);
    }
    if (i < min(max(nq[t], 0), qcap) && inView[(int64_t)t * qcap + i]) {                        // :1168
        const int p = queries[(int64_t)t * qcap + i];
        if (td_in(p, npoints)) atomicAdd(&visible[p], 1);
    }
}

__global__ __launch_bounds__(TD_T) void k_td_mark(int cap, int nframes, const int32_t* n, const int32_t* frame, const int32_t* slots,
                                                 const uint8_t* outlier, const int32_t* after, int npoints, int words, uint32_t* bits)
{
    const int t = blockIdx.y, i = blockIdx.x * TD_T + threadIdx.x;
    int f;
    if (i >= td_frame(n, frame, t, nframes, cap, f)) return;
    const int p = slots[(int64_t)t * cap + i];
    // discarded: flagged, or no longer in its slot after PoseOptimization's discard (which clears the flags it acts on)
    const bool gone = (outlier && outlier[(int64_t)t * cap + i]) || (after && after[(int64_t)t * cap + i] != p);
    if (gone && td_in(p, npoints)) atomicOr(&bits[(int64_t)t * words + (p >> 5)], 1u << (p & 31));
}

__global__ __launch_bounds__(TD_T) void k_td_seen(int qcap, const int32_t* nq, const int32_t* queries, int npoints, int words,
                                                 const uint32_t* bits, uint8_t* seen)
{
    const int t = blockIdx.y, i = blockIdx.x * TD_T + threadIdx.x;
    if (i >= min(max(nq[t], 0), qcap)) return;
    const int p = queries[(int64_t)t * qcap + i];
    seen[(int64_t)t * qcap + i] = td_in(p, npoints) ? (bits[(int64_t)t * words + (p >> 5)] >> (p & 31)) & 1u : 0;
}

struct TdDecide {
    int mode; const int32_t* modes; int afterRetry, cap, nframes; const int32_t* n; const int32_t* frame; const uint8_t* run;
    const int32_t* nmatches; const int32_t* nmatchesMap; const pgorb_kf_pose* poseBefore; const int32_t* slotsBefore;
    const pgorb_kf_pose* poseOpt; const int32_t* slotsOpt; const uint8_t* outlier; int npoints; const uint8_t* hasObs; int32_t* found;
    const pgorb_track_counters* counters; uint8_t* ok; int32_t* inliers; uint8_t* retry; pgorb_kf_pose* poseFinal; int32_t* slotsFinal;
};

__global__ __launch_bounds__(TD_T) void k_td_decide(TdDecide A)
{
    __shared__ int sh[TD_W];
    const int t = blockIdx.x;
    if (A.run && !A.run[t]) {                                                                   // TrackLocalMap did not run: bOK stays false
        if (threadIdx.x == 0) A.ok[t] = 0;
        return;
    }
    const int m = A.modes ? A.modes[t] : A.mode;
    int f;
    const int n = td_frame(A.n, A.frame, t, A.nframes, A.cap, f);
    const int64_t row = (int64_t)t * A.cap;
    bool ok = false, opt = false;
    if (m == PGORB_DECIDE_LOCAL_MAP) {                                                          // :932-964
        int c = 0;
        for (int i = threadIdx.x; i < n; i += TD_T) {
            const int p = A.slotsOpt[row + i];
            if (!td_in(p, A.npoints) || A.outlier[row + i]) continue;
            if (A.found) atomicAdd(&A.found[p], 1);                                             // IncreaseFound()
            c += !A.hasObs || A.hasObs[p];                                                      // Observations() > 0
        }
        const int inl = td_block_sum(c, sh);
        const pgorb_track_counters C = A.counters[t];
        ok = !(C.frame_id < td_sum(C.last_reloc_frame_id, C.max_frames) && inl < 50) && inl >= 30;
        opt = true;
        if (threadIdx.x == 0) A.inliers[t] = inl;
    } else if (m == PGORB_DECIDE_REFERENCE_KF) {                                                // :760, :789
        opt = A.nmatches[t] >= 15;
        ok = opt && A.nmatchesMap[t] >= 10;
    } else if (m == PGORB_DECIDE_MOTION_MODEL) {                                                // :879-886, :918
        opt = A.nmatches[t] >= 20;
        ok = opt && A.nmatchesMap[t] >= 10;
        if (threadIdx.x == 0) A.retry[t] = !A.afterRetry && !opt;
    } else {
        if (threadIdx.x == 0) A.ok[t] = 0;
        return;
    }
    if (threadIdx.x == 0) {
        A.ok[t] = ok;
        A.poseFinal[t] = opt ? A.poseOpt[t] : A.poseBefore[t];
    }
    const int32_t* src = opt ? A.slotsOpt : A.slotsBefore;
    for (int i = threadIdx.x; i < n; i += TD_T) A.slotsFinal[row + i] = src[row + i];
}

struct TdFinish {
    int cap, nframes; const int32_t* n; const int32_t* frame; const uint8_t* ok; const int32_t* inliers; pgorb_track_counters* counters;
    const pgorb_kf_pose* poseFinal; const int32_t* slots; uint8_t* outlier; const uint8_t* hasObs; TdObs O;
    int32_t* kfPoint; pgorb_kf_pose* kfPose; uint64_t* kfId; int32_t* slotsOut; int32_t* refKfOut; int32_t* newKf; uint8_t* interruptBa;
};

__global__ __launch_bounds__(TD_T) void k_td_finish(TdFinish A)
{
    __shared__ int sh[TD_W];
    const int t = blockIdx.x;
    int f;
    const int n = td_frame(A.n, A.frame, t, A.nframes, A.cap, f);
    const int64_t row = (int64_t)t * A.cap;
    pgorb_track_counters C = A.counters[t];
    if (!A.ok[t]) {                                                                             // :429: nothing of the tail runs
        for (int i = threadIdx.x; i < n; i += TD_T) A.slotsOut[row + i] = A.slots[row + i];
        if (threadIdx.x == 0) { A.refKfOut[t] = C.ref_kf; A.newKf[t] = -1; A.interruptBa[t] = 0; }
        return;
    }
    // NeedNewKeyFrame (:968-1052), monocular.  The early returns are the same in every lane, so the count below is too.
    const bool early = C.stopped || C.stop_requested || (C.frame_id < td_sum(C.last_reloc_frame_id, C.max_frames) && C.nkfs > C.max_frames);
    int nRef = 0;
    if (!early) {
        const int r = C.ref_kf, nr = td_in(r, A.nframes) ? min(max(A.n[r], 0), A.cap) : 0;
        nRef = td_block_sum(td_tracked(A.O, A.kfPoint + (int64_t)r * A.cap, nr, C.nkfs <= 2 ? 2 : 3), sh);
    }
    bool need = false;
    if (!early) {
        const int inl = A.inliers[t];
        const bool idle = C.accept_keyframes != 0;
        const bool c1a = C.frame_id >= td_sum(C.last_kf_frame_id, C.max_frames);
        const bool c1b = C.frame_id >= td_sum(C.last_kf_frame_id, C.min_frames) && idle;
        const bool c2 = (float)inl < __fmul_rn((float)nRef, 0.9f) && inl > 15;                  // int < int * float: one float product
        need = (c1a || c1b) && c2;
    }
    const bool create = need && C.accept_keyframes && C.set_not_stop_ok && td_in(f, A.nframes);
    for (int i = threadIdx.x; i < n; i += TD_T) {
        int p = A.slots[row + i];
        uint8_t o = A.outlier[row + i];
        if (td_in(p, A.O.npoints) && A.hasObs && !A.hasObs[p]) {                                // clean VO matches (:445-454)
            p = -1; o = 0;
            A.outlier[row + i] = 0;
        }
        if (create) A.kfPoint[(int64_t)f * A.cap + i] = p;                                      // KeyFrame(mCurrentFrame, ..): outliers included
        if (td_in(p, A.O.npoints) && o) p = -1;                                                 // :472-476
        A.slotsOut[row + i] = p;
    }
    if (threadIdx.x == 0) {
        if (create) {                                                                           // :1059-1062, :1130
            A.kfPose[f] = A.poseFinal[t];
            A.kfId[f] = C.next_kf_id;
            C.next_kf_id += 1; C.ref_kf = f; C.last_kf_frame_id = (uint32_t)C.frame_id; C.nkfs += 1;
            A.counters[t] = C;
        }
        A.refKfOut[t] = C.ref_kf;
        A.newKf[t] = create ? f : -1;
        A.interruptBa[t] = need && !C.accept_keyframes;                                         // InterruptBA() (:1038), reported
    }
}

// ---- ComputeSceneMedianDepth (KeyFrame.cc:736-766)
extern __shared__ uint32_t td_lds[];                                                           // keys [cap], hist [TD_W][256], misc [8]
static inline size_t td_lds_bytes(int cap) { return ((size_t)cap + TD_W * 256 + 8) * 4; }

// vDepths[(size - 1) / q] of one row after std::sort, in every lane; *status = 0, PGORB_DEPTH_EMPTY or PGORB_DEPTH_NAN (then -1.0f).
// A key is the float's bits made monotone (negative: all bits flipped, else the sign bit set); a slot without a point takes
// 0xFFFFFFFF, above +inf and, once NaNs are ruled out, no depth's key, so it sorts behind every depth and is never chosen.
__device__ float td_median(const int32_t* rowp, int n, const float* T, const pgorb_map_point* pts, int npoints, int q, int cap, int* status)
{
    uint32_t* keys = td_lds;
    uint32_t* hist = td_lds + cap;
    uint32_t* misc = hist + TD_W * 256;
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < 8) misc[tid] = 0;
    __syncthreads();
    int c = 0, nan = 0;
    for (int i = tid; i < n; i += TD_T) {
        const int p = rowp[i];
        uint32_t key = 0xFFFFFFFFu;
        if (td_in(p, npoints)) {                                                                // no isBad() test (:754)
            float z = cnm_f(__dadd_rn(cnm_dotd(T[8], T[9], T[10], pts[p].pos[0], pts[p].pos[1], pts[p].pos[2]), (double)T[11]));
            if (z != z) nan = 1;
            else {
                uint32_t u = __float_as_uint(z);
                if ((u << 1) == 0) u = 0;                                                       // operator< cannot tell -0 from +0
                key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                c++;
            }
        }
        keys[i] = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_down(c, o); nan |= __shfl_down(nan, o); }
    if ((tid & 63) == 0) { atomicAdd(&misc[0], (uint32_t)c); atomicOr(&misc[1], (uint32_t)nan); }
    __syncthreads();
    const uint32_t count = misc[0];
    if (misc[1]) { *status = PGORB_DEPTH_NAN; return -1.0f; }
    if (!count) { *status = PGORB_DEPTH_EMPTY; return -1.0f; }
    *status = 0;
    uint32_t k = (count - 1) / (uint32_t)max(q, 1), prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = tid; j < TD_W * 256; j += TD_T) hist[j] = 0;
        __syncthreads();
        uint32_t* mine = hist + (tid >> 6) * 256;
        for (int i = tid; i < n; i += TD_T) {
            const uint32_t key = keys[i];
            if ((key & mask) == prefix) atomicAdd(&mine[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        uint32_t h = 0;
#pragma unroll
        for (int w = 0; w < TD_W; w++) h += hist[w * 256 + (tid & 255)];
        __syncthreads();
        hist[tid & 255] = h;
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            int d = 0;
            for (; d < 255 && k >= acc + hist[d]; d++) acc += hist[d];
            misc[2] = (uint32_t)d; misc[3] = k - acc;
        }
        __syncthreads();
        prefix |= misc[2] << shift; mask |= 255u << shift; k = misc[3];
        __syncthreads();
    }
    return __uint_as_float((prefix & 0x80000000u) ? (prefix ^ 0x80000000u) : ~prefix);
}

__global__ __launch_bounds__(TD_T) void k_td_median(int nlist, const int32_t* list, int q, const int32_t* kfPoint, const int32_t* n, int nframes,
                                                   int cap, const pgorb_kf_pose* pose, int npoints, const pgorb_map_point* pts, float* out,
                                                   int32_t* status)
{
    const int kf = list[blockIdx.x];
    if (!td_in(kf, nframes)) return;
    int st;
    const float m = td_median(kfPoint + (int64_t)kf * cap, min(max(n[kf], 0), cap), pose[kf].Tcw, pts, npoints, q, cap, &st);
    if (threadIdx.x == 0) { out[blockIdx.x] = m; status[blockIdx.x] = st; }
}

// ---- CreateInitialMapMonocular's scale (Tracking.cc:684-709)
__global__ __launch_bounds__(TD_T) void k_td_scale_head(int kfIni, int kfCur, const int32_t* kfPoint, const int32_t* n, int cap, pgorb_kf_pose* pose,
                                                       const pgorb_map_point* pts, TdObs O, int32_t* info)
{
    __shared__ int sh[TD_W];
    int st = PGORB_DEPTH_EMPTY;
    float med = -1.0f;
    if (td_in(kfIni, O.nframes))
        med = td_median(kfPoint + (int64_t)kfIni * cap, min(max(n[kfIni], 0), cap), pose[kfIni].Tcw, pts, O.npoints, 2, cap, &st);
    const int nc = td_in(kfCur, O.nframes) ? min(max(n[kfCur], 0), cap) : 0;
    const int tracked = td_block_sum(td_tracked(O, kfPoint + (int64_t)kfCur * cap, nc, 1), sh);
    if (threadIdx.x) return;
    const bool wrong = med < 0.0f || tracked < 100;                                             // :688
    info[0] = st | (wrong ? PGORB_DECIDE_WRONG_INIT : 0);
    info[1] = __float_as_int(med); info[2] = tracked; info[3] = 0;
    if (wrong) return;
    const float inv = __fdiv_rn(1.0f, med);
    pgorb_kf_pose P = pose[kfCur];
    P.Tcw[3] = __fmul_rn(P.Tcw[3], inv); P.Tcw[7] = __fmul_rn(P.Tcw[7], inv); P.Tcw[11] = __fmul_rn(P.Tcw[11], inv);   // :697
    po_set_ow(P);                                                                               // SetPose (:698)
    pose[kfCur] = P;
}

__global__ __launch_bounds__(TD_T) void k_td_scale_count(int kfIni, const int32_t* kfPoint, const int32_t* n, int nframes, int cap, int npoints,
                                                        const int32_t* info, int32_t* held)
{
    const int i = blockIdx.x * TD_T + threadIdx.x;
    if ((info[0] & PGORB_DECIDE_WRONG_INIT) || !td_in(kfIni, nframes) || i >= min(max(n[kfIni], 0), cap)) return;
    const int p = kfPoint[(int64_t)kfIni * cap + i];
    if (td_in(p, npoints)) atomicAdd(&held[p], 1);
}

__global__ __launch_bounds__(TD_T) void k_td_scale_points(int npoints, pgorb_map_point* pts, const int32_t* held, int32_t* info)
{
    const int p = blockIdx.x * TD_T + threadIdx.x;
    if ((info[0] & PGORB_DECIDE_WRONG_INIT) || p >= npoints) return;
    const int c = held[p];
    if (!c) return;
    const float inv = __fdiv_rn(1.0f, __int_as_float(info[1]));
    float x = pts[p].pos[0], y = pts[p].pos[1], z = pts[p].pos[2];
    for (int k = 0; k < c; k++) { x = __fmul_rn(x, inv); y = __fmul_rn(y, inv); z = __fmul_rn(z, inv); }   // once per slot that holds it (:702-709)
    pts[p].pos[0] = x; pts[p].pos[1] = y; pts[p].pos[2] = z;
    atomicAdd(&info[3], 1);
}

static inline unsigned td_blocks(int n) { return (unsigned)((std::max(n, 1) + TD_T - 1) / TD_T); }
static inline size_t td_up(size_t b) { return (b + 63) & ~(size_t)63; }

#define TD_FAIL(code, msg) return pg_ctx_fail(c, code, msg)
#define TD_DEVICE() if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) TD_FAIL(PGORB_E_HIP, "hipSetDevice failed")
#define TD_LAUNCHED(name) if (hipGetLastError() != hipSuccess) TD_FAIL(PGORB_E_HIP, name " launch failed")

extern "C" {

int pgorb_check_replaced_batch_device(pgorb_ctx* c, int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame,
        int32_t* d_last_point, int npoints, const int32_t* d_replaced, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0 || (ntrack && (!d_n || (cap_per_frame && !d_last_point) || (npoints && !d_replaced))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_check_replaced_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_check_replaced: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame");
    TD_DEVICE();
    if (!ntrack || !cap_per_frame) return 0;
    hipLaunchKernelGGL(k_td_replaced, dim3(td_blocks(cap_per_frame), ntrack), dim3(TD_T), 0, (hipStream_t)stream, cap_per_frame, nframes, d_n, d_frame,
                       d_last_point, npoints, d_replaced);
    TD_LAUNCHED("k_td_replaced");
    return 0;
}

int pgorb_increase_visible_batch_device(pgorb_ctx* c, int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame,
        const uint8_t* d_run, const int32_t* d_kp_point, int qcap, const int32_t* d_nq, const int32_t* d_queries, const uint8_t* d_in_view,
        int npoints, int32_t* d_visible, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (ntrack < 0 || nframes < 0 || cap_per_frame < 0 || qcap < 0 || npoints < 0 ||
        (ntrack && (!d_n || !d_nq || (cap_per_frame && !d_kp_point) || (qcap && (!d_queries || !d_in_view)) || (npoints && !d_visible))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_increase_visible_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000 || qcap > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_increase_visible: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames, 16000 keypoints per frame or 16000 queries");
    TD_DEVICE();
    if (!ntrack || !npoints || !(cap_per_frame || qcap)) return 0;
    hipLaunchKernelGGL(k_td_visible, dim3(td_blocks(std::max(cap_per_frame, qcap)), ntrack), dim3(TD_T), 0, (hipStream_t)stream, cap_per_frame, nframes,
                       d_n, d_frame, d_run, d_kp_point, qcap, d_nq, d_queries, d_in_view, npoints, d_visible);
    TD_LAUNCHED("k_td_visible");
    return 0;
}

int pgorb_query_seen_from_outliers_batch_device(pgorb_ctx* c, int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame,
        const int32_t* d_kp_point, const uint8_t* d_outlier, const int32_t* d_kp_point_opt, int qcap, const int32_t* d_nq, const int32_t* d_queries,
        int npoints, uint8_t* d_query_seen, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (ntrack < 0 || nframes < 0 || cap_per_frame < 0 || qcap < 0 || npoints < 0 ||
        (ntrack && (!d_n || !d_nq || (cap_per_frame && (!d_kp_point || (!d_outlier && !d_kp_point_opt))) || (qcap && (!d_queries || !d_query_seen)))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_query_seen_from_outliers_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000 || qcap > 16000 || npoints > TD_SEEN_MAX_POINTS)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_query_seen_from_outliers: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames, 16000 keypoints per frame, 16000 queries or 1048576 points");
    TD_DEVICE();
    if (!ntrack || !qcap) return 0;
    const hipStream_t s = (hipStream_t)stream;
    const int words = (npoints + 31) / 32 + 1;
    void* p;
    int rc = pg_ctx_scratch(c, td_up((size_t)ntrack * words * 4), s, &p);
    if (rc) return rc;
    if (hipMemsetAsync(p, 0, (size_t)ntrack * words * 4, s) != hipSuccess) { pg_ctx_scratch_done(c, s); TD_FAIL(PGORB_E_HIP, "hipMemsetAsync failed"); }
    if (cap_per_frame)
        hipLaunchKernelGGL(k_td_mark, dim3(td_blocks(cap_per_frame), ntrack), dim3(TD_T), 0, s, cap_per_frame, nframes, d_n, d_frame, d_kp_point, d_outlier,
                           d_kp_point_opt, npoints, words, (uint32_t*)p);
    hipLaunchKernelGGL(k_td_seen, dim3(td_blocks(qcap), ntrack), dim3(TD_T), 0, s, qcap, d_nq, d_queries, npoints, words, (const uint32_t*)p, d_query_seen);
    if (hipGetLastError() != hipSuccess) { pg_ctx_scratch_done(c, s); TD_FAIL(PGORB_E_HIP, "k_td_mark / k_td_seen launch failed"); }
    return pg_ctx_scratch_done(c, s);
}

int pgorb_track_decide_batch_device(pgorb_ctx* c, int ntrack, int mode, const int32_t* d_mode, int after_retry, const int32_t* d_n, int nframes,
        int cap_per_frame, const int32_t* d_frame, const uint8_t* d_run, const int32_t* d_nmatches, const int32_t* d_nmatches_map,
        const pgorb_kf_pose* d_pose_before, const int32_t* d_kp_point_before, const pgorb_kf_pose* d_pose_opt, const int32_t* d_kp_point_opt,
        const uint8_t* d_outlier, int npoints, const uint8_t* d_point_has_obs, int32_t* d_found, const pgorb_track_counters* d_counters,
        uint8_t* d_ok, int32_t* d_inliers, uint8_t* d_retry, pgorb_kf_pose* d_pose_final, int32_t* d_kp_point_final, void* stream)
{
    if (!c) return PGORB_E_ARG;
    const bool first = d_mode || mode != PGORB_DECIDE_LOCAL_MAP, local = d_mode || mode == PGORB_DECIDE_LOCAL_MAP;
    if (ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0 ||
        (!d_mode && mode != PGORB_DECIDE_MOTION_MODEL && mode != PGORB_DECIDE_REFERENCE_KF && mode != PGORB_DECIDE_LOCAL_MAP) ||
        (ntrack && (!d_n || !d_ok || !d_pose_final || !d_pose_opt || (cap_per_frame && (!d_kp_point_opt || !d_kp_point_final)) ||
                    (first && (!d_nmatches || !d_nmatches_map || !d_pose_before || !d_retry || (cap_per_frame && !d_kp_point_before))) ||
                    (local && (!d_counters || !d_inliers || (cap_per_frame && !d_outlier))))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_track_decide_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_track_decide: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame");
    TD_DEVICE();
    if (!ntrack) return 0;
    const TdDecide A = {mode, d_mode, after_retry != 0, cap_per_frame, nframes, d_n, d_frame, d_run, d_nmatches, d_nmatches_map, d_pose_before,
                        d_kp_point_before, d_pose_opt, d_kp_point_opt, d_outlier, npoints, d_point_has_obs, d_found, d_counters, d_ok, d_inliers,
                        d_retry, d_pose_final, d_kp_point_final};
    hipLaunchKernelGGL(k_td_decide, dim3(ntrack), dim3(TD_T), 0, (hipStream_t)stream, A);
    TD_LAUNCHED("k_td_decide");
    return 0;
}

int pgorb_track_finish_batch_device(pgorb_ctx* c, int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame,
        const uint8_t* d_ok, const int32_t* d_inliers, pgorb_track_counters* d_counters, const pgorb_kf_pose* d_pose_final,
        const int32_t* d_kp_point, uint8_t* d_outlier, int npoints, const uint8_t* d_point_bad, const uint8_t* d_point_has_obs,
        const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint8_t* d_obs_live, int32_t* d_kf_point, pgorb_kf_pose* d_kf_pose,
        uint64_t* d_kf_id, int32_t* d_kp_point_out, int32_t* d_ref_kf_out, int32_t* d_new_kf, uint8_t* d_interrupt_ba, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0 || nobs < 0 ||
        (ntrack && (!d_n || !d_ok || !d_inliers || !d_counters || !d_pose_final || !d_ref_kf_out || !d_new_kf || !d_interrupt_ba ||
                    (cap_per_frame && (!d_kp_point || !d_outlier || !d_kp_point_out)) || (npoints && !d_obs_start) || (nobs && !d_obs_frame) ||
                    (nframes && (!d_kf_pose || !d_kf_id || (cap_per_frame && !d_kf_point))))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_track_finish_batch_device");
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_track_finish: more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame");
    TD_DEVICE();
    if (!ntrack) return 0;
    const TdFinish A = {cap_per_frame, nframes, d_n, d_frame, d_ok, d_inliers, d_counters, d_pose_final, d_kp_point, d_outlier, d_point_has_obs,
                        {npoints, d_point_bad, d_obs_start, d_obs_frame, nobs, d_obs_live, nframes}, d_kf_point, d_kf_pose, d_kf_id, d_kp_point_out,
                        d_ref_kf_out, d_new_kf, d_interrupt_ba};
    hipLaunchKernelGGL(k_td_finish, dim3(ntrack), dim3(TD_T), 0, (hipStream_t)stream, A);
    TD_LAUNCHED("k_td_finish");
    return 0;
}

int pgorb_scene_median_depth_batch_device(pgorb_ctx* c, int nlist, const int32_t* d_kf, int q, const int32_t* d_kf_point, const int32_t* d_n,
        int nframes, int cap_per_frame, const pgorb_kf_pose* d_pose, int npoints, const pgorb_map_point* d_points, float* d_median_depth,
        int32_t* d_status, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nlist < 0 || q < 1 || nframes < 0 || cap_per_frame < 0 || npoints < 0 ||
        (nlist && (!d_kf || !d_median_depth || !d_status || (nframes && (!d_n || !d_pose || (cap_per_frame && !d_kf_point))) || (npoints && !d_points))))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_scene_median_depth_batch_device");
    if (nlist > PGORB_DEPTH_MAX_LIST || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_scene_median_depth: more than PGORB_DEPTH_MAX_LIST entries, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame");
    TD_DEVICE();
    if (!nlist) return 0;
    const size_t lds = td_lds_bytes(cap_per_frame);
    if (!pg_raise_lds<k_td_median>(c, lds)) TD_FAIL(PGORB_E_LIMIT, "pgorb_scene_median_depth: the keys do not fit the LDS");
    hipLaunchKernelGGL(k_td_median, dim3(nlist), dim3(TD_T), lds, (hipStream_t)stream, nlist, d_kf, q, d_kf_point, d_n, nframes, cap_per_frame, d_pose,
                       npoints, d_points, d_median_depth, d_status);
    TD_LAUNCHED("k_td_median");
    return 0;
}

int pgorb_scale_initial_map_device(pgorb_ctx* c, int kf_ini, int kf_cur, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame,
        pgorb_kf_pose* d_pose, int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start,
        const int32_t* d_obs_frame, int nobs, const uint8_t* d_obs_live, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap_per_frame < 0 || npoints < 0 || nobs < 0 || !d_info || (nframes && (!d_n || !d_pose || (cap_per_frame && !d_kf_point))) ||
        (npoints && (!d_points || !d_obs_start)) || (nobs && !d_obs_frame))
        TD_FAIL(PGORB_E_ARG, "bad argument to pgorb_scale_initial_map_device");
    if (nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000 || npoints > (1 << 30))
        TD_FAIL(PGORB_E_LIMIT, "pgorb_scale_initial_map: more than PGORB_COVIS_MAX_KF frames, 16000 keypoints per frame or 2^30 points");
    TD_DEVICE();
    const hipStream_t s = (hipStream_t)stream;
    const size_t lds = td_lds_bytes(cap_per_frame);
    if (!pg_raise_lds<k_td_scale_head>(c, lds)) TD_FAIL(PGORB_E_LIMIT, "pgorb_scale_initial_map: the keys do not fit the LDS");
    void* p;
    int rc = pg_ctx_scratch(c, td_up((size_t)std::max(npoints, 1) * 4), s, &p);
    if (rc) return rc;
    if (hipMemsetAsync(p, 0, (size_t)std::max(npoints, 1) * 4, s) != hipSuccess) { pg_ctx_scratch_done(c, s); TD_FAIL(PGORB_E_HIP, "hipMemsetAsync failed"); }
    const TdObs O = {npoints, d_point_bad, d_obs_start, d_obs_frame, nobs, d_obs_live, nframes};
    hipLaunchKernelGGL(k_td_scale_head, dim3(1), dim3(TD_T), lds, s, kf_ini, kf_cur, d_kf_point, d_n, cap_per_frame, d_pose, d_points, O, d_info);
    if (cap_per_frame && npoints) {
        hipLaunchKernelGGL(k_td_scale_count, dim3(td_blocks(cap_per_frame)), dim3(TD_T), 0, s, kf_ini, d_kf_point, d_n, nframes, cap_per_frame, npoints,
                           d_info, (int32_t*)p);
        hipLaunchKernelGGL(k_td_scale_points, dim3(td_blocks(npoints)), dim3(TD_T), 0, s, npoints, d_points, (const int32_t*)p, d_info);
    }
    if (hipGetLastError() != hipSuccess) { pg_ctx_scratch_done(c, s); TD_FAIL(PGORB_E_HIP, "k_td_scale_head / k_td_scale_count / k_td_scale_points launch failed"); }
    return pg_ctx_scratch_done(c, s);
}

// ---- the host forms: the same flat arrays in host memory, checked, then one synchronous call of the device form
struct TdCheck {
    const char* fn; const char* why = nullptr;
    explicit TdCheck(const char* f) : fn(f) {}
    void no(bool bad, const char* w) { if (bad && !why) why = w; }
    // a [rows][stride] array of table indices whose first count[row] entries lie in [lo, hi)
    void rows(const int32_t* a, int rows_, int stride, const std::vector<int>& count, int lo, int hi, const char* w)
    {
        for (int t = 0; !why && t < rows_; t++)
            for (int i = 0; i < count[t]; i++)
                if (a[(size_t)t * stride + i] < lo || a[(size_t)t * stride + i] >= hi) { why = w; break; }
    }
    int fail(pgorb_ctx* c, int code = PGORB_E_ARG) const { return pg_ctx_fail(c, code, (std::string(fn) + ": " + why).c_str()); }
};

// the slot count of every tracker, or false
static bool td_counts(TdCheck& K, int ntrack, const int32_t* n, int nframes, int cap, const int32_t* frame, std::vector<int>& count)
{
    count.assign((size_t)std::max(ntrack, 0), 0);
    for (int f = 0; f < nframes && !K.why; f++) K.no(n[f] < 0 || n[f] > cap, "a frame's count is outside [0, cap_per_frame]");
    for (int t = 0; t < ntrack && !K.why; t++) {
        const int f = frame ? frame[t] : t;
        K.no(f < 0 || f >= nframes, "a tracker's frame is out of range");
        if (!K.why) count[t] = n[f];
    }
    return !K.why;
}

static bool td_obs_ok(TdCheck& K, int npoints, const int32_t* start, const int32_t* frame, int nobs, const uint8_t* live, int nframes)
{
    if (npoints) {
        K.no(start[0] != 0 || start[npoints] != nobs, "obs_start does not run from 0 to nobs");
        for (int p = 0; p < npoints && !K.why; p++) K.no(start[p + 1] < start[p], "obs_start is not rising");
    } else K.no(nobs != 0, "observations without points");
    for (int j = 0; j < nobs && !K.why; j++) K.no((!live || live[j]) && (frame[j] < 0 || frame[j] >= nframes), "a live observation names a frame out of range");
    return !K.why;
}

#define TD_LIMITS(fn) \
    if (ntrack > PGORB_TRACK_MAX || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000) \
        TD_FAIL(PGORB_E_LIMIT, fn ": more than PGORB_TRACK_MAX trackers, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame")

int pgorb_check_replaced(pgorb_ctx* c, int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, int32_t* last_point,
        int npoints, const int32_t* replaced)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_check_replaced");
    K.no(ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0, "a count is negative");
    K.no(!n || !last_point || !replaced, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    TD_LIMITS("pgorb_check_replaced");
    std::vector<int> cnt;
    if (td_counts(K, ntrack, n, nframes, cap_per_frame, frame, cnt)) {
        K.rows(last_point, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        for (int p = 0; p < npoints && !K.why; p++) K.no(replaced[p] < -1 || replaced[p] >= npoints, "a replacement is out of range");
    }
    if (K.why) return K.fail(c);
    const size_t T = (size_t)std::max(ntrack, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), NP = (size_t)std::max(npoints, 1);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, F * 4), oF = s.region(PG_UP, T * 4), oR = s.region(PG_UP, NP * 4), oL = s.region(PG_INOUT, T * cap * 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, n, (size_t)nframes * 4, 0, F * 4); s.put(oF, frame, (size_t)ntrack * 4, 0, T * 4); s.put(oR, replaced, (size_t)npoints * 4, 0, NP * 4);
    s.put(oL, last_point, (size_t)ntrack * cap_per_frame * 4, 0, T * cap * 4);
    if ((rc = s.run([&] { return pgorb_check_replaced_batch_device(c, ntrack, s.dev<int32_t>(oN), nframes, cap_per_frame, frame ? s.dev<int32_t>(oF) : nullptr,
                                                                   s.dev<int32_t>(oL), npoints, s.dev<int32_t>(oR), nullptr); }))) return rc;
    memcpy(last_point, s.host(oL), (size_t)ntrack * cap_per_frame * 4);
    return 0;
}

int pgorb_increase_visible(pgorb_ctx* c, int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, const uint8_t* run,
        const int32_t* kp_point, int qcap, const int32_t* nq, const int32_t* queries, const uint8_t* in_view, int npoints, int32_t* visible)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_increase_visible");
    K.no(ntrack < 0 || nframes < 0 || cap_per_frame < 0 || qcap < 0 || npoints < 0, "a count is negative");
    K.no(!n || !kp_point || !nq || !queries || !in_view || !visible, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    TD_LIMITS("pgorb_increase_visible");
    if (qcap > 16000) TD_FAIL(PGORB_E_LIMIT, "pgorb_increase_visible: more than 16000 queries");
    std::vector<int> cnt, qn((size_t)ntrack, 0);
    if (td_counts(K, ntrack, n, nframes, cap_per_frame, frame, cnt)) {
        for (int t = 0; t < ntrack && !K.why; t++) { K.no(nq[t] < 0 || nq[t] > qcap, "a query count is outside [0, qcap]"); qn[t] = nq[t]; }
        K.rows(kp_point, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        if (!K.why) K.rows(queries, ntrack, qcap, qn, 0, npoints, "a query names a point out of range");
    }
    if (K.why) return K.fail(c);
    const size_t T = (size_t)std::max(ntrack, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), Q = (size_t)std::max(qcap, 1),
                 NP = (size_t)std::max(npoints, 1);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, F * 4), oF = s.region(PG_UP, T * 4), oRun = s.region(PG_UP, T), oS = s.region(PG_UP, T * cap * 4), oNq = s.region(PG_UP, T * 4),
                 oQ = s.region(PG_UP, T * Q * 4), oIv = s.region(PG_UP, T * Q), oV = s.region(PG_INOUT, NP * 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, n, (size_t)nframes * 4, 0, F * 4); s.put(oF, frame, (size_t)ntrack * 4, 0, T * 4); s.put(oRun, run, (size_t)ntrack, 0, T);
    s.put(oS, kp_point, (size_t)ntrack * cap_per_frame * 4, 0, T * cap * 4); s.put(oNq, nq, (size_t)ntrack * 4, 0, T * 4);
    s.put(oQ, queries, (size_t)ntrack * qcap * 4, 0, T * Q * 4); s.put(oIv, in_view, (size_t)ntrack * qcap, 0, T * Q);
    s.put(oV, visible, (size_t)npoints * 4, 0, NP * 4);
    if ((rc = s.run([&] { return pgorb_increase_visible_batch_device(c, ntrack, s.dev<int32_t>(oN), nframes, cap_per_frame, frame ? s.dev<int32_t>(oF) : nullptr,
            run ? s.dev(oRun) : nullptr, s.dev<int32_t>(oS), qcap, s.dev<int32_t>(oNq), s.dev<int32_t>(oQ), s.dev(oIv), npoints, s.dev<int32_t>(oV), nullptr); })))
        return rc;
    memcpy(visible, s.host(oV), (size_t)npoints * 4);
    return 0;
}

int pgorb_query_seen_from_outliers(pgorb_ctx* c, int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame,
        const int32_t* kp_point, const uint8_t* outlier, const int32_t* kp_point_opt, int qcap, const int32_t* nq, const int32_t* queries, int npoints,
        uint8_t* query_seen)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_query_seen_from_outliers");
    K.no(ntrack < 0 || nframes < 0 || cap_per_frame < 0 || qcap < 0 || npoints < 0, "a count is negative");
    K.no(!n || !kp_point || (!outlier && !kp_point_opt) || !nq || !queries || !query_seen, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    TD_LIMITS("pgorb_query_seen_from_outliers");
    if (qcap > 16000 || npoints > TD_SEEN_MAX_POINTS) TD_FAIL(PGORB_E_LIMIT, "pgorb_query_seen_from_outliers: more than 16000 queries or 1048576 points");
    std::vector<int> cnt, qn((size_t)ntrack, 0);
    if (td_counts(K, ntrack, n, nframes, cap_per_frame, frame, cnt)) {
        for (int t = 0; t < ntrack && !K.why; t++) { K.no(nq[t] < 0 || nq[t] > qcap, "a query count is outside [0, qcap]"); qn[t] = nq[t]; }
        K.rows(kp_point, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        if (!K.why && kp_point_opt) K.rows(kp_point_opt, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        if (!K.why) K.rows(queries, ntrack, qcap, qn, 0, npoints, "a query names a point out of range");
    }
    if (K.why) return K.fail(c);
    const size_t T = (size_t)std::max(ntrack, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), Q = (size_t)std::max(qcap, 1);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, F * 4), oF = s.region(PG_UP, T * 4), oS = s.region(PG_UP, T * cap * 4), oO = s.region(PG_UP, T * cap),
                 oA = s.region(PG_UP, T * cap * 4),
                 oNq = s.region(PG_UP, T * 4), oQ = s.region(PG_UP, T * Q * 4), oSeen = s.region(PG_INOUT, T * Q);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, n, (size_t)nframes * 4, 0, F * 4); s.put(oF, frame, (size_t)ntrack * 4, 0, T * 4);
    s.put(oS, kp_point, (size_t)ntrack * cap_per_frame * 4, 0, T * cap * 4); s.put(oO, outlier, (size_t)ntrack * cap_per_frame, 0, T * cap);
    s.put(oA, kp_point_opt, (size_t)ntrack * cap_per_frame * 4, 0, T * cap * 4);
    s.put(oNq, nq, (size_t)ntrack * 4, 0, T * 4); s.put(oQ, queries, (size_t)ntrack * qcap * 4, 0, T * Q * 4);
    s.put(oSeen, query_seen, (size_t)ntrack * qcap, 0, T * Q);
    if ((rc = s.run([&] { return pgorb_query_seen_from_outliers_batch_device(c, ntrack, s.dev<int32_t>(oN), nframes, cap_per_frame,
            frame ? s.dev<int32_t>(oF) : nullptr, s.dev<int32_t>(oS), outlier ? s.dev(oO) : nullptr, kp_point_opt ? s.dev<int32_t>(oA) : nullptr, qcap, s.dev<int32_t>(oNq), s.dev<int32_t>(oQ), npoints, s.dev(oSeen), nullptr); })))
        return rc;
    memcpy(query_seen, s.host(oSeen), (size_t)ntrack * qcap);
    return 0;
}

int pgorb_track_decide(pgorb_ctx* c, int ntrack, int mode, const int32_t* modes, int after_retry, const int32_t* n, int nframes, int cap_per_frame,
        const int32_t* frame, const uint8_t* run, const int32_t* nmatches, const int32_t* nmatches_map, const pgorb_kf_pose* pose_before,
        const int32_t* kp_point_before, const pgorb_kf_pose* pose_opt, const int32_t* kp_point_opt, const uint8_t* outlier, int npoints,
        const uint8_t* point_has_obs, int32_t* found, const pgorb_track_counters* counters, uint8_t* ok, int32_t* inliers, uint8_t* retry,
        pgorb_kf_pose* pose_final, int32_t* kp_point_final)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_track_decide");
    K.no(ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0, "a count is negative");
    K.no(!n || !nmatches || !nmatches_map || !pose_before || !kp_point_before || !pose_opt || !kp_point_opt || !outlier || !found || !counters || !ok ||
         !inliers || !retry || !pose_final || !kp_point_final, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    TD_LIMITS("pgorb_track_decide");
    for (int t = 0; !K.why && t < ntrack; t++) {
        const int m = modes ? modes[t] : mode;
        K.no(m != PGORB_DECIDE_MOTION_MODEL && m != PGORB_DECIDE_REFERENCE_KF && m != PGORB_DECIDE_LOCAL_MAP, "an unknown mode");
    }
    if (K.why) return K.fail(c);
    std::vector<int> cnt;
    if (td_counts(K, ntrack, n, nframes, cap_per_frame, frame, cnt)) {
        K.rows(kp_point_before, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        if (!K.why) K.rows(kp_point_opt, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
    }
    if (K.why) return K.fail(c);
    const size_t T = (size_t)std::max(ntrack, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), NP = (size_t)std::max(npoints, 1),
                 pb = sizeof(pgorb_kf_pose), cb = sizeof(pgorb_track_counters);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, F * 4), oF = s.region(PG_UP, T * 4), oM = s.region(PG_UP, T * 4), oRun = s.region(PG_UP, T), oNm = s.region(PG_UP, T * 4),
                 oMap = s.region(PG_UP, T * 4), oPb = s.region(PG_UP, T * pb), oSb = s.region(PG_UP, T * cap * 4), oPo = s.region(PG_UP, T * pb),
                 oSo = s.region(PG_UP, T * cap * 4), oOut = s.region(PG_UP, T * cap), oHas = s.region(PG_UP, NP), oC = s.region(PG_UP, T * cb),
                 oFound = s.region(PG_INOUT, NP * 4), oOk = s.region(PG_INOUT, T), oInl = s.region(PG_INOUT, T * 4), oRetry = s.region(PG_INOUT, T),
                 oPf = s.region(PG_INOUT, T * pb), oSf = s.region(PG_INOUT, T * cap * 4);
    int rc = s.begin();
    if (rc) return rc;
    const size_t tc = (size_t)ntrack * cap_per_frame;
    s.put(oN, n, (size_t)nframes * 4, 0, F * 4); s.put(oF, frame, (size_t)ntrack * 4, 0, T * 4); s.put(oM, modes, (size_t)ntrack * 4, 0, T * 4);
    s.put(oRun, run, (size_t)ntrack, 0, T); s.put(oNm, nmatches, (size_t)ntrack * 4, 0, T * 4); s.put(oMap, nmatches_map, (size_t)ntrack * 4, 0, T * 4);
    s.put(oPb, pose_before, (size_t)ntrack * pb, 0, T * pb); s.put(oSb, kp_point_before, tc * 4, 0, T * cap * 4); s.put(oPo, pose_opt, (size_t)ntrack * pb, 0, T * pb);
    s.put(oSo, kp_point_opt, tc * 4, 0, T * cap * 4); s.put(oOut, outlier, tc, 0, T * cap); s.put(oHas, point_has_obs, (size_t)npoints, 0, NP);
    s.put(oC, counters, (size_t)ntrack * cb, 0, T * cb); s.put(oFound, found, (size_t)npoints * 4, 0, NP * 4); s.put(oOk, ok, (size_t)ntrack, 0, T);
    s.put(oInl, inliers, (size_t)ntrack * 4, 0, T * 4); s.put(oRetry, retry, (size_t)ntrack, 0, T); s.put(oPf, pose_final, (size_t)ntrack * pb, 0, T * pb);
    s.put(oSf, kp_point_final, tc * 4, 0, T * cap * 4);
    if ((rc = s.run([&] { return pgorb_track_decide_batch_device(c, ntrack, mode, modes ? s.dev<int32_t>(oM) : nullptr, after_retry, s.dev<int32_t>(oN), nframes,
            cap_per_frame, frame ? s.dev<int32_t>(oF) : nullptr, run ? s.dev(oRun) : nullptr, s.dev<int32_t>(oNm), s.dev<int32_t>(oMap), s.dev<pgorb_kf_pose>(oPb),
            s.dev<int32_t>(oSb), s.dev<pgorb_kf_pose>(oPo), s.dev<int32_t>(oSo), s.dev(oOut), npoints, point_has_obs ? s.dev(oHas) : nullptr, s.dev<int32_t>(oFound),
            s.dev<pgorb_track_counters>(oC), s.dev(oOk), s.dev<int32_t>(oInl), s.dev(oRetry), s.dev<pgorb_kf_pose>(oPf), s.dev<int32_t>(oSf), nullptr); })))
        return rc;
    memcpy(found, s.host(oFound), (size_t)npoints * 4); memcpy(ok, s.host(oOk), (size_t)ntrack); memcpy(inliers, s.host(oInl), (size_t)ntrack * 4);
    memcpy(retry, s.host(oRetry), (size_t)ntrack); memcpy(pose_final, s.host(oPf), (size_t)ntrack * pb); memcpy(kp_point_final, s.host(oSf), tc * 4);
    return 0;
}

int pgorb_track_finish(pgorb_ctx* c, int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, const uint8_t* ok,
        const int32_t* inliers, pgorb_track_counters* counters, const pgorb_kf_pose* pose_final, const int32_t* kp_point, uint8_t* outlier, int npoints,
        const uint8_t* point_bad, const uint8_t* point_has_obs, const int32_t* obs_start, const int32_t* obs_frame, int nobs, const uint8_t* obs_live,
        int32_t* kf_point, pgorb_kf_pose* kf_pose, uint64_t* kf_id, int32_t* kp_point_out, int32_t* ref_kf_out, int32_t* new_kf, uint8_t* interrupt_ba)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_track_finish");
    K.no(ntrack < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0 || nobs < 0, "a count is negative");
    K.no(!n || !ok || !inliers || !counters || !pose_final || !kp_point || !outlier || !obs_start || !obs_frame || !kf_point || !kf_pose || !kf_id ||
         !kp_point_out || !ref_kf_out || !new_kf || !interrupt_ba, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    TD_LIMITS("pgorb_track_finish");
    std::vector<int> cnt;
    if (td_counts(K, ntrack, n, nframes, cap_per_frame, frame, cnt) && td_obs_ok(K, npoints, obs_start, obs_frame, nobs, obs_live, nframes)) {
        K.rows(kp_point, ntrack, cap_per_frame, cnt, -1, npoints, "a slot names a point out of range");
        std::set<int> rows;
        for (int t = 0; t < ntrack && !K.why; t++) K.no(!rows.insert(frame ? frame[t] : t).second, "two trackers name one frame row");
        for (int t = 0; t < ntrack && !K.why; t++) {
            const int r = counters[t].ref_kf;
            K.no(r < 0 || r >= nframes, "a reference key frame is out of range");
            K.no(rows.count(r) != 0, "a reference key frame is a tracker's frame row");
            if (K.why) break;
            for (int i = 0; i < n[r]; i++)
                if (kf_point[(size_t)r * cap_per_frame + i] < -1 || kf_point[(size_t)r * cap_per_frame + i] >= npoints) { K.why = "a key frame's slot names a point out of range"; break; }
        }
    }
    if (K.why) return K.fail(c);
    const size_t T = (size_t)std::max(ntrack, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), NP = (size_t)std::max(npoints, 1),
                 NO = (size_t)std::max(nobs, 1), pb = sizeof(pgorb_kf_pose), cb = sizeof(pgorb_track_counters), tc = (size_t)ntrack * cap_per_frame,
                 fc = (size_t)nframes * cap_per_frame;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, F * 4), oF = s.region(PG_UP, T * 4), oOk = s.region(PG_UP, T), oInl = s.region(PG_UP, T * 4), oPf = s.region(PG_UP, T * pb),
                 oS = s.region(PG_UP, T * cap * 4), oBad = s.region(PG_UP, NP), oHas = s.region(PG_UP, NP), oSt = s.region(PG_UP, (NP + 1) * 4),
                 oOf = s.region(PG_UP, NO * 4), oLive = s.region(PG_UP, NO), oC = s.region(PG_INOUT, T * cb), oOut = s.region(PG_INOUT, T * cap),
                 oKp = s.region(PG_INOUT, F * cap * 4), oKpose = s.region(PG_INOUT, F * pb), oKid = s.region(PG_INOUT, F * 8), oSo = s.region(PG_INOUT, T * cap * 4),
                 oRef = s.region(PG_INOUT, T * 4), oNew = s.region(PG_INOUT, T * 4), oInt = s.region(PG_INOUT, T);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, n, (size_t)nframes * 4, 0, F * 4); s.put(oF, frame, (size_t)ntrack * 4, 0, T * 4); s.put(oOk, ok, (size_t)ntrack, 0, T);
    s.put(oInl, inliers, (size_t)ntrack * 4, 0, T * 4); s.put(oPf, pose_final, (size_t)ntrack * pb, 0, T * pb); s.put(oS, kp_point, tc * 4, 0, T * cap * 4);
    s.put(oBad, point_bad, (size_t)npoints, 0, NP); s.put(oHas, point_has_obs, (size_t)npoints, 0, NP);
    s.put(oSt, obs_start, (size_t)(npoints + 1) * 4, 0, (NP + 1) * 4); s.put(oOf, obs_frame, (size_t)nobs * 4, 0, NO * 4); s.put(oLive, obs_live, (size_t)nobs, 0, NO);
    s.put(oC, counters, (size_t)ntrack * cb, 0, T * cb); s.put(oOut, outlier, tc, 0, T * cap); s.put(oKp, kf_point, fc * 4, 0, F * cap * 4);
    s.put(oKpose, kf_pose, (size_t)nframes * pb, 0, F * pb); s.put(oKid, kf_id, (size_t)nframes * 8, 0, F * 8); s.put(oSo, kp_point_out, tc * 4, 0, T * cap * 4);
    s.put(oRef, ref_kf_out, (size_t)ntrack * 4, 0, T * 4); s.put(oNew, new_kf, (size_t)ntrack * 4, 0, T * 4); s.put(oInt, interrupt_ba, (size_t)ntrack, 0, T);
    if ((rc = s.run([&] { return pgorb_track_finish_batch_device(c, ntrack, s.dev<int32_t>(oN), nframes, cap_per_frame, frame ? s.dev<int32_t>(oF) : nullptr,
            s.dev(oOk), s.dev<int32_t>(oInl), s.dev<pgorb_track_counters>(oC), s.dev<pgorb_kf_pose>(oPf), s.dev<int32_t>(oS), s.dev(oOut), npoints,
            point_bad ? s.dev(oBad) : nullptr, point_has_obs ? s.dev(oHas) : nullptr, s.dev<int32_t>(oSt), s.dev<int32_t>(oOf), nobs, obs_live ? s.dev(oLive) : nullptr,
            s.dev<int32_t>(oKp), s.dev<pgorb_kf_pose>(oKpose), s.dev<uint64_t>(oKid), s.dev<int32_t>(oSo), s.dev<int32_t>(oRef), s.dev<int32_t>(oNew), s.dev(oInt),
            nullptr); }))) return rc;
    memcpy(counters, s.host(oC), (size_t)ntrack * cb); memcpy(outlier, s.host(oOut), tc); memcpy(kf_point, s.host(oKp), fc * 4);
    memcpy(kf_pose, s.host(oKpose), (size_t)nframes * pb); memcpy(kf_id, s.host(oKid), (size_t)nframes * 8); memcpy(kp_point_out, s.host(oSo), tc * 4);
    memcpy(ref_kf_out, s.host(oRef), (size_t)ntrack * 4); memcpy(new_kf, s.host(oNew), (size_t)ntrack * 4); memcpy(interrupt_ba, s.host(oInt), (size_t)ntrack);
    int made = 0;
    for (int t = 0; t < ntrack; t++) made += new_kf[t] >= 0;
    return made;
}

int pgorb_scene_median_depth(pgorb_ctx* c, int nlist, const int32_t* kf, int q, const int32_t* kf_point, const int32_t* n, int nframes, int cap_per_frame,
        const pgorb_kf_pose* pose, int npoints, const pgorb_map_point* points, float* median_depth, int32_t* status)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_scene_median_depth");
    K.no(nlist < 0 || nframes < 0 || cap_per_frame < 0 || npoints < 0, "a count is negative");
    K.no(q < 1, "q is not positive");
    K.no(!kf || !kf_point || !n || !pose || !points || !median_depth || !status, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    if (nlist > PGORB_DEPTH_MAX_LIST || nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000)
        TD_FAIL(PGORB_E_LIMIT, "pgorb_scene_median_depth: more than PGORB_DEPTH_MAX_LIST entries, PGORB_COVIS_MAX_KF frames or 16000 keypoints per frame");
    for (int f = 0; f < nframes && !K.why; f++) {
        K.no(n[f] < 0 || n[f] > cap_per_frame, "a frame's count is outside [0, cap_per_frame]");
        for (int i = 0; !K.why && i < n[f]; i++)
            K.no(kf_point[(size_t)f * cap_per_frame + i] < -1 || kf_point[(size_t)f * cap_per_frame + i] >= npoints, "a slot names a point out of range");
    }
    for (int e = 0; e < nlist && !K.why; e++) K.no(kf[e] < -1 || kf[e] >= nframes, "a key frame is out of range");
    if (K.why) return K.fail(c);
    const size_t L = (size_t)std::max(nlist, 1), F = (size_t)std::max(nframes, 1), cap = (size_t)std::max(cap_per_frame, 1), NP = (size_t)std::max(npoints, 1),
                 pb = sizeof(pgorb_kf_pose), mb = sizeof(pgorb_map_point), fc = (size_t)nframes * cap_per_frame;
    PgHostCall s(c);
    const size_t oL = s.region(PG_UP, L * 4), oKp = s.region(PG_UP, F * cap * 4), oN = s.region(PG_UP, F * 4), oP = s.region(PG_UP, F * pb),
                 oPts = s.region(PG_UP, NP * mb), oM = s.region(PG_INOUT, L * 4), oSt = s.region(PG_INOUT, L * 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oL, kf, (size_t)nlist * 4, 0, L * 4); s.put(oKp, kf_point, fc * 4, 0, F * cap * 4); s.put(oN, n, (size_t)nframes * 4, 0, F * 4);
    s.put(oP, pose, (size_t)nframes * pb, 0, F * pb); s.put(oPts, points, (size_t)npoints * mb, 0, NP * mb);
    s.put(oM, median_depth, (size_t)nlist * 4, 0, L * 4); s.put(oSt, status, (size_t)nlist * 4, 0, L * 4);
    if ((rc = s.run([&] { return pgorb_scene_median_depth_batch_device(c, nlist, s.dev<int32_t>(oL), q, s.dev<int32_t>(oKp), s.dev<int32_t>(oN), nframes,
            cap_per_frame, s.dev<pgorb_kf_pose>(oP), npoints, s.dev<pgorb_map_point>(oPts), s.dev<float>(oM), s.dev<int32_t>(oSt), nullptr); }))) return rc;
    memcpy(median_depth, s.host(oM), (size_t)nlist * 4); memcpy(status, s.host(oSt), (size_t)nlist * 4);
    return 0;
}

int pgorb_scale_initial_map(pgorb_ctx* c, int kf_ini, int kf_cur, const int32_t* kf_point, const int32_t* n, int nframes, int cap_per_frame,
        pgorb_kf_pose* pose, int npoints, pgorb_map_point* points, const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame, int nobs,
        const uint8_t* obs_live, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    TdCheck K("pgorb_scale_initial_map");
    K.no(nframes < 0 || cap_per_frame < 0 || npoints < 0 || nobs < 0, "a count is negative");
    K.no(!kf_point || !n || !pose || !points || !obs_start || !obs_frame || !info, "an array that is read or written is NULL");
    if (K.why) return K.fail(c);
    if (nframes > PGORB_COVIS_MAX_KF || cap_per_frame > 16000 || npoints > (1 << 30))
        TD_FAIL(PGORB_E_LIMIT, "pgorb_scale_initial_map: more than PGORB_COVIS_MAX_KF frames, 16000 keypoints per frame or 2^30 points");
    K.no(kf_ini < 0 || kf_ini >= nframes || kf_cur < 0 || kf_cur >= nframes || kf_ini == kf_cur, "a key frame is out of range, or both are one");
    for (int f = 0; f < nframes && !K.why; f++) {
        K.no(n[f] < 0 || n[f] > cap_per_frame, "a frame's count is outside [0, cap_per_frame]");
        for (int i = 0; !K.why && i < n[f]; i++)
            K.no(kf_point[(size_t)f * cap_per_frame + i] < -1 || kf_point[(size_t)f * cap_per_frame + i] >= npoints, "a slot names a point out of range");
    }
    if (!K.why) td_obs_ok(K, npoints, obs_start, obs_frame, nobs, obs_live, nframes);
    if (K.why) return K.fail(c);
    const size_t F = (size_t)nframes, cap = (size_t)std::max(cap_per_frame, 1), NP = (size_t)std::max(npoints, 1), NO = (size_t)std::max(nobs, 1),
                 pb = sizeof(pgorb_kf_pose), mb = sizeof(pgorb_map_point), fc = (size_t)nframes * cap_per_frame;
    PgHostCall s(c);
    const size_t oKp = s.region(PG_UP, F * cap * 4), oN = s.region(PG_UP, F * 4), oBad = s.region(PG_UP, NP), oSt = s.region(PG_UP, (NP + 1) * 4),
                 oOf = s.region(PG_UP, NO * 4), oLive = s.region(PG_UP, NO), oP = s.region(PG_INOUT, F * pb), oPts = s.region(PG_INOUT, NP * mb),
                 oInfo = s.region(PG_DOWN, 64);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oKp, kf_point, fc * 4, 0, F * cap * 4); s.put(oN, n, F * 4); s.put(oBad, point_bad, (size_t)npoints, 0, NP);
    s.put(oSt, obs_start, (size_t)(npoints + 1) * 4, 0, (NP + 1) * 4); s.put(oOf, obs_frame, (size_t)nobs * 4, 0, NO * 4); s.put(oLive, obs_live, (size_t)nobs, 0, NO);
    s.put(oP, pose, F * pb); s.put(oPts, points, (size_t)npoints * mb, 0, NP * mb);
    if ((rc = s.run([&] { return pgorb_scale_initial_map_device(c, kf_ini, kf_cur, s.dev<int32_t>(oKp), s.dev<int32_t>(oN), nframes, cap_per_frame,
            s.dev<pgorb_kf_pose>(oP), npoints, s.dev<pgorb_map_point>(oPts), point_bad ? s.dev(oBad) : nullptr, s.dev<int32_t>(oSt), s.dev<int32_t>(oOf), nobs,
            obs_live ? s.dev(oLive) : nullptr, s.dev<int32_t>(oInfo), nullptr); }))) return rc;
    memcpy(pose, s.host(oP), F * pb); memcpy(points, s.host(oPts), (size_t)npoints * mb); memcpy(info, s.host(oInfo), PGORB_DECIDE_INFO * 4);
    return (info[0] & PGORB_DECIDE_WRONG_INIT) ? 0 : info[3];
}

}  // extern "C"
