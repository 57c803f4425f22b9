// map_point.hip -- the per-point refresh at the end of the local-mapping functions, for many map points in one call, on gfx950.
//
// Restates (thirdparty/orb-slam2):
//   MapPoint::ComputeDistinctiveDescriptors   src/MapPoint.cc:259-324
//   MapPoint::UpdateNormalAndDepth            src/MapPoint.cc:347-388
//   their call sites                          src/LocalMapping.cc:444-446, 519-532 (and :152-153, Optimizer.cc:776, Tracking.cc:533-534)
//
// A point's observation list is given in the order the caller's mObservations iterates (a std::map<KeyFrame*, size_t>: address
// order, which the library cannot know): the list order IS the contract, for the first-smallest-median rule and for the float sum.
//   k_mp_bin        one lane per selected point: the no-ops (bad, empty), the limit, and the rest binned by list length n
//   k_mp_seg<SEG>   n <= SEG: a segment of SEG lanes per point, 64 / SEG points per wave; lane l owns observation l: its
//                   descriptor in 8 VGPRs, its row of distances in SEG VGPRs (descriptor j comes from lane j), the row's
//                   (int)(0.5*(N-1))-th smallest by a 9-step bisection on the value, the winner a segment minimum of
//                   (median << 16) | l.  N <= 2 needs no distance: both medians are the rows' own 0 and the first candidate wins.
//   k_mp_big        64 < n <= PGORB_MP_MAX_OBS: a workgroup per point, the descriptors in LDS, a thread per row
// The normal's terms are formed one per lane and added serially in list order; every float operation follows the reference's
// cv::Mat arithmetic under the readings of DESIGN.md section 4 (cnm_normd / cnm_f of match_common.h).
#include "loop_pose.h"                     // mp_term, mp_depth: shared with loop_correct.hip

#define MP_CLASSES 5                       // n <= 2, 8, 32, 64, PGORB_MP_MAX_OBS
#define MP_BIG_T 256
#define MP_NOT_CAND 0x3FF                  // "distance" to an observation that is no candidate: above every real one (<= 256)

struct PgMpBatch {
    const pgorb_keypoint* K; const uint8_t* D; const int32_t* n; int cap; int nframes;
    const pgorb_kf_pose* pose; const uint8_t* kfBad;
    int npoints; pgorb_map_point* pts; uint8_t* pdesc; const uint8_t* pbad;
    const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs; const int32_t* refObs;
    int nsel; const int32_t* select; int what;
    int32_t* bestObs; int32_t* status;
    float sf[PG_MAXL + 1]; int nlevels;
};

__device__ __forceinline__ int mp_class(int n) { return n <= 2 ? 0 : n <= 8 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : 4; }

// bins[c][0 .. cnt[c]) = the selection positions of class c, in any order (the points are independent)
__global__ __launch_bounds__(256) void k_mp_bin(PgMpBatch B, int32_t* __restrict__ cnt, int32_t* __restrict__ bins)
{
    const int s = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int cls = -1;
    if (s < B.nsel) {
        const int p = B.select ? B.select[s] : s;
        int st = 0;
        if (p < 0 || p >= B.npoints) st = PGORB_MP_BAD_INDEX;
        else if (!(B.pbad && B.pbad[p])) {                                   // :268-269, :355-356
            const int a = B.obsStart[p], b = B.obsStart[p + 1];
            if (a < 0 || b < a || b > B.nobs) st = PGORB_MP_BAD_INDEX;
            else if (b - a > PGORB_MP_MAX_OBS) st = PGORB_MP_LIMIT;
            else if (b > a) cls = mp_class(b - a);                           // (empty: :273-274, :362-363)
        }
        if (cls < 0) { B.status[s] = st; if (B.bestObs) B.bestObs[s] = -1; }
    }
    for (int c = 0; c < MP_CLASSES; c++) {                                   // one atomic per wave and class
        const unsigned long long m = __ballot(cls == c);
        if (!m) continue;
        int base = 0;
        if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&cnt[c], __popcll(m));
        base = __shfl(base, __ffsll((long long)m) - 1);
        if (cls == c) bins[(int64_t)c * B.nsel + base + __popcll(m & ((1ull << lane) - 1))] = s;
    }
}

// observation (f, i) names a keypoint of the batch
__device__ __forceinline__ bool mp_obs_ok(const PgMpBatch& B, int f, int i)
{
    return f >= 0 && f < B.nframes && i >= 0 && i < min(B.n[f], B.cap);
}

// minimum over the SEG lanes of a segment, in every lane: quad permutes and row mirrors on DPP, the halves above 16 by shuffles
template <int SEG> __device__ __forceinline__ unsigned mp_seg_min(unsigned x)
{
    int v = (int)x;
    if (SEG >= 2) v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    if (SEG >= 4) v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    if (SEG >= 8) v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));   // row_half_mirror
    if (SEG >= 16) v = (int)min((unsigned)v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));  // row_mirror
    if (SEG >= 32) v = (int)min((unsigned)v, (unsigned)__shfl_xor(v, 16));
    if (SEG >= 64) v = (int)min((unsigned)v, (unsigned)__shfl_xor(v, 32));
    return (unsigned)v;
}

template <int SEG> __global__ __launch_bounds__(256) void k_mp_seg(PgMpBatch B, const int32_t* __restrict__ cnt, const int32_t* __restrict__ bin)
{
    constexpr int PPW = 64 / SEG;
    const int lane = threadIdx.x & 63, l = lane & (SEG - 1), segBase = lane & ~(SEG - 1);
    const int count = min(*cnt, B.nsel);
    const int item = (blockIdx.x * 4 + (threadIdx.x >> 6)) * PPW + lane / SEG;
    if (item - lane / SEG >= count) return;                                   // the whole wave
    const unsigned long long segMask = (SEG == 64 ? ~0ull : ((1ull << (SEG & 63)) - 1)) << segBase;
    const bool active = item < count;
    int s = 0, p = 0, a = 0, n = 0;
    if (active) { s = bin[item]; p = B.select ? B.select[s] : s; a = B.obsStart[p]; n = B.obsStart[p + 1] - a; }
    const bool inList = l < n;
    int f = 0, i = 0;
    if (inList) { f = B.obsFrame[a + l]; i = B.obsIdx[a + l]; }
    const bool ok = inList && mp_obs_ok(B, f, i);
    const int r = (active && (B.what & PGORB_MP_NORMAL_DEPTH)) ? B.refObs[p] : 0;
    bool live = active && !(__ballot(inList && !ok) & segMask) && r >= 0 && r < n;
    if (active && !live && l == 0) { B.status[s] = PGORB_MP_BAD_INDEX; if (B.bestObs) B.bestObs[s] = -1; }
    const bool cand = live && ok && !(B.kfBad && B.kfBad[f]);                 // :278-284
    const unsigned long long cb = __ballot(cand) & segMask;
    const int N = __popcll(cb);
    int st = 0, best = -1;
    if (B.what & PGORB_MP_DESCRIPTOR) {
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        if (cand) {
            const uint4* d = reinterpret_cast<const uint4*>(B.D + ((int64_t)f * B.cap + i) * 32);
            q0 = d[0]; q1 = d[1];
        }
        unsigned med = 0;
        if (SEG > 2 && __any(N > 2)) {
            int d[SEG];
#pragma unroll
            for (int j = 0; j < SEG; j++) {                                   // Distances[l][j] (:293-302)
                const int src = segBase + j;
                const uint4 o0 = make_uint4(__shfl(q0.x, src), __shfl(q0.y, src), __shfl(q0.z, src), __shfl(q0.w, src));
                const uint4 o1 = make_uint4(__shfl(q1.x, src), __shfl(q1.y, src), __shfl(q1.z, src), __shfl(q1.w, src));
                d[j] = ((cb >> src) & 1) ? pg_hamming256(q0, q1, o0, o1) : MP_NOT_CAND;
            }
            const int k = (N - 1) >> 1;                                       // vDists[0.5*(N-1)] (:311)
            int lo = 0, hi = 256;
            for (int it = 0; it < 9; it++) {                                  // the smallest v with #{j : d[j] <= v} > k
                const int mid = (lo + hi) >> 1;
                int c = 0;
#pragma unroll
                for (int j = 0; j < SEG; j++) c += d[j] <= mid;
                if (c > k) hi = mid; else lo = mid + 1;
            }
            med = (unsigned)lo;
        }
        const unsigned key = mp_seg_min<SEG>(cand ? (med << 16) | (unsigned)l : 0xFFFFFFFFu);   // median < BestMedian (:313): the first wins
        if (N > 0) {
            best = (int)(key & 0xFFFF);
            st |= PGORB_MP_DESCRIPTOR;
            if (l == best) {
                uint4* o = reinterpret_cast<uint4*>(B.pdesc + (int64_t)p * 32);
                o[0] = q0; o[1] = q1;
            }
        }
    }
    if (B.what & PGORB_MP_NORMAL_DEPTH) {                                     // every observation, bad key frames included (:367-374)
        float t[3] = {0.f, 0.f, 0.f};
        if (live && inList) {
            const float* pos = B.pts[p].pos;
            double nd;
            mp_term(pos, B.pose[f].Ow, t, nd);
            if (l == r) {
                float mn, mx;
                mp_depth(B.sf, B.nlevels, nd, B.K[(int64_t)f * B.cap + i].octave, mn, mx);
                B.pts[p].min_distance = mn; B.pts[p].max_distance = mx;
            }
        }
        float sx = 0.f, sy = 0.f, sz = 0.f;                                   // normal = normal + term, in list order
#pragma unroll
        for (int j = 0; j < SEG; j++) {
            const float tx = __shfl(t[0], segBase + j), ty = __shfl(t[1], segBase + j), tz = __shfl(t[2], segBase + j);
            if (j < n) { sx = __fadd_rn(sx, tx); sy = __fadd_rn(sy, ty); sz = __fadd_rn(sz, tz); }
        }
        if (live && l == 0) {
            const float sc = cnm_f(__ddiv_rn(1.0, (double)n));                // normal/n
            B.pts[p].normal[0] = __fmul_rn(sx, sc); B.pts[p].normal[1] = __fmul_rn(sy, sc); B.pts[p].normal[2] = __fmul_rn(sz, sc);
        }
        st |= PGORB_MP_NORMAL_DEPTH;
    }
    if (live && l == 0) { B.status[s] = st; if (B.bestObs) B.bestObs[s] = best; }
}

__global__ __launch_bounds__(MP_BIG_T) void k_mp_big(PgMpBatch B, const int32_t* __restrict__ cnt, const int32_t* __restrict__ bin)
{
    __shared__ uint4 sD[2 * PGORB_MP_MAX_OBS];
    __shared__ float sT[3][PGORB_MP_MAX_OBS];
    __shared__ uint8_t sC[PGORB_MP_MAX_OBS];
    __shared__ int sN, sInvalid;
    __shared__ unsigned sKey;
    __shared__ float sMin, sMax;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= min(*cnt, B.nsel)) return;
    const int s = bin[blockIdx.x], p = B.select ? B.select[s] : s;
    const int a = B.obsStart[p], n = B.obsStart[p + 1] - a;
    const int r = (B.what & PGORB_MP_NORMAL_DEPTH) ? B.refObs[p] : 0;
    if (tid == 0) { sN = 0; sInvalid = (r < 0 || r >= n); sKey = 0xFFFFFFFFu; }
    __syncthreads();
    for (int l = tid; l < n; l += MP_BIG_T) {
        const int f = B.obsFrame[a + l], i = B.obsIdx[a + l];
        const bool ok = mp_obs_ok(B, f, i);
        const bool cand = ok && !(B.kfBad && B.kfBad[f]);
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        float t[3] = {0.f, 0.f, 0.f};
        if (!ok) sInvalid = 1;
        else {
            if (cand && (B.what & PGORB_MP_DESCRIPTOR)) {
                const uint4* d = reinterpret_cast<const uint4*>(B.D + ((int64_t)f * B.cap + i) * 32);
                q0 = d[0]; q1 = d[1];
            }
            if (B.what & PGORB_MP_NORMAL_DEPTH) {
                double nd;
                mp_term(B.pts[p].pos, B.pose[f].Ow, t, nd);
                if (l == r) { float mn, mx; mp_depth(B.sf, B.nlevels, nd, B.K[(int64_t)f * B.cap + i].octave, mn, mx); sMin = mn; sMax = mx; }
            }
        }
        sD[2 * l] = q0; sD[2 * l + 1] = q1;
        sT[0][l] = t[0]; sT[1][l] = t[1]; sT[2][l] = t[2];
        sC[l] = cand;
        if (cand) atomicAdd(&sN, 1);
    }
    __syncthreads();
    if (sInvalid) {
        if (tid == 0) { B.status[s] = PGORB_MP_BAD_INDEX; if (B.bestObs) B.bestObs[s] = -1; }
        return;
    }
    const int N = sN;
    int st = 0, best = -1;
    if ((B.what & PGORB_MP_DESCRIPTOR) && N > 0) {
        const int k = (N - 1) >> 1;
        for (int l = tid; l < n; l += MP_BIG_T) {
            if (!sC[l]) continue;
            unsigned med = 0;
            if (N > 2) {
                const uint4 q0 = sD[2 * l], q1 = sD[2 * l + 1];
                int lo = 0, hi = 256;
                for (int it = 0; it < 9; it++) {
                    const int mid = (lo + hi) >> 1;
                    int c = 0;
                    for (int j = 0; j < n; j++) c += (sC[j] ? pg_hamming256(q0, q1, sD[2 * j], sD[2 * j + 1]) : MP_NOT_CAND) <= mid;
                    if (c > k) hi = mid; else lo = mid + 1;
                }
                med = (unsigned)lo;
            }
            atomicMin(&sKey, (med << 16) | (unsigned)l);
        }
        __syncthreads();
        best = (int)(sKey & 0xFFFF);
        st |= PGORB_MP_DESCRIPTOR;
        if (tid < 2) reinterpret_cast<uint4*>(B.pdesc + (int64_t)p * 32)[tid] = sD[2 * best + tid];
    }
    if (B.what & PGORB_MP_NORMAL_DEPTH) {
        st |= PGORB_MP_NORMAL_DEPTH;
        if (tid < 3) {                                                        // a lane per component, the terms in list order
            float sum = 0.f;
            for (int j = 0; j < n; j++) sum = __fadd_rn(sum, sT[tid][j]);
            B.pts[p].normal[tid] = __fmul_rn(sum, cnm_f(__ddiv_rn(1.0, (double)n)));
        }
        if (tid == 3) { B.pts[p].min_distance = sMin; B.pts[p].max_distance = sMax; }
    }
    if (tid == 0) { B.status[s] = st; if (B.bestObs) B.bestObs[s] = best; }
}

template <int SEG> static void mp_launch_seg(const PgMpBatch& B, const int32_t* cnt, const int32_t* bins, int cls, hipStream_t s)
{
    const int waves = (B.nsel + 64 / SEG - 1) / (64 / SEG);
    hipLaunchKernelGGL(k_mp_seg<SEG>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, B, cnt + cls, bins + (int64_t)cls * B.nsel);
}

extern "C" {

int pgorb_refresh_map_points_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int nframes,
                                          int cap, const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, int npoints,
                                          pgorb_map_point* d_points, uint8_t* d_point_desc, const uint8_t* d_point_bad,
                                          const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
                                          const int32_t* d_ref_obs, int nsel, const int32_t* d_select, int what, int32_t* d_best_obs,
                                          int32_t* d_status, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || nsel < 0 || what < 1 || what > PGORB_MP_BOTH ||
        (nframes && (!d_kps || !d_desc || !d_n || !d_pose)) || (npoints && (!d_points || !d_point_desc || !d_obs_start)) ||
        (nobs && (!d_obs_frame || !d_obs_idx)) || (nsel && !d_status) || (npoints && (what & PGORB_MP_NORMAL_DEPTH) && !d_ref_obs))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_refresh_map_points_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!nsel) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    PgMpBatch B = {d_kps, d_desc, d_n, cap, nframes, d_pose, d_kf_bad, npoints, d_points, d_point_desc, d_point_bad, d_obs_start,
                   d_obs_frame, d_obs_idx, nobs, d_ref_obs, nsel, d_select, what, d_best_obs, d_status};
    pgorb_scale_tables(c, B.sf, nullptr, nullptr, nullptr);
    B.nlevels = pgorb_levels(c);
    if (B.nlevels < 1) return pg_ctx_fail(c, PGORB_E_ARG, "context has no levels");
    void* scr;
    int rc = pg_ctx_scratch(c, 256 + (size_t)MP_CLASSES * nsel * 4, s, &scr);
    if (rc) return rc;
    int32_t* cnt = (int32_t*)scr;
    int32_t* bins = (int32_t*)((uint8_t*)scr + 256);
    if (hipMemsetAsync(cnt, 0, 256, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_mp_bin, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, s, B, cnt, bins);
    mp_launch_seg<2>(B, cnt, bins, 0, s);
    mp_launch_seg<8>(B, cnt, bins, 1, s);
    mp_launch_seg<32>(B, cnt, bins, 2, s);
    mp_launch_seg<64>(B, cnt, bins, 3, s);
    hipLaunchKernelGGL(k_mp_big, dim3((unsigned)nsel), dim3(MP_BIG_T), 0, s, B, (const int32_t*)(cnt + 4), (const int32_t*)(bins + (int64_t)4 * nsel));
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_mp_bin / k_mp_seg / k_mp_big launch failed");
    return pg_ctx_scratch_done(c, s);
}

// host buffers: a one-problem batch of the device form; the inputs are checked here
int pgorb_refresh_map_points(pgorb_ctx* c, int nkf, const pgorb_keypoint* const* kps, const uint8_t* const* desc, const int32_t* n,
                             const pgorb_kf_pose* pose, const uint8_t* kf_bad, int npoints, pgorb_map_point* points, uint8_t* point_desc,
                             const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx,
                             const int32_t* ref_obs, int nsel, const int32_t* select, int what, int32_t* best_obs, int32_t* status)
{
    if (!c) return PGORB_E_ARG;
    const char* bad = "bad argument to pgorb_refresh_map_points";
    if (nkf < 0 || npoints < 0 || nsel < 0 || what < 1 || what > PGORB_MP_BOTH || !obs_start || (nkf && (!kps || !desc || !n || !pose)) ||
        (npoints && (!points || !point_desc)) || (nsel && !status) || (!select && nsel != npoints) ||
        (npoints && (what & PGORB_MP_NORMAL_DEPTH) && !ref_obs))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    int cap = 1;
    for (int f = 0; f < nkf; f++) {
        if (n[f] < 0 || (n[f] && (!kps[f] || !desc[f]))) return pg_ctx_fail(c, PGORB_E_ARG, bad);
        if (n[f] > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        cap = std::max(cap, n[f]);
    }
    if (obs_start[0] != 0) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: obs_start[0] must be 0");
    for (int i = 0; i < npoints; i++)
        if (obs_start[i + 1] < obs_start[i]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: obs_start decreases");
    const int nobs = obs_start[npoints];
    if (nobs && (!obs_frame || !obs_idx)) return pg_ctx_fail(c, PGORB_E_ARG, bad);
    for (int k = 0; k < nobs; k++)
        if (obs_frame[k] < 0 || obs_frame[k] >= nkf || obs_idx[k] < 0 || obs_idx[k] >= n[obs_frame[k]])
            return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: an observation names a key frame or keypoint out of range");
    std::vector<int32_t> seen((size_t)std::max(nkf, 1), -1);
    for (int i = 0; i < npoints; i++)
        for (int k = obs_start[i]; k < obs_start[i + 1]; k++) {
            if (seen[obs_frame[k]] == i) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: a list names a key frame twice");
            seen[obs_frame[k]] = i;
        }
    std::vector<uint8_t> chosen((size_t)std::max(npoints, 1), 0);
    for (int q = 0; q < nsel; q++) {
        const int p = select ? select[q] : q;
        if (p < 0 || p >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: a selection index is out of range");
        if (chosen[p]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: a point is selected twice");
        chosen[p] = 1;
        const int len = obs_start[p + 1] - obs_start[p];
        if ((what & PGORB_MP_NORMAL_DEPTH) && !(point_bad && point_bad[p]) && len > 0 && len <= PGORB_MP_MAX_OBS &&
            (ref_obs[p] < 0 || ref_obs[p] >= len))
            return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_refresh_map_points: ref_obs lies outside the point's list");
    }
    if (!nsel) return 0;
    const int np = std::max(npoints, 1), no = std::max(nobs, 1), nf = std::max(nkf, 1);
    const size_t kb = sizeof(pgorb_keypoint);
    PgHostCall hc(c);
    const size_t oK = hc.region(PG_UP, (size_t)nf * cap * kb), oD = hc.region(PG_UP, (size_t)nf * cap * 32), oN = hc.region(PG_UP, (size_t)nf * 4),
                 oPose = hc.region(PG_UP, (size_t)nf * sizeof(pgorb_kf_pose)), oKB = hc.region(PG_UP, nf), oB = hc.region(PG_UP, np),
                 oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = hc.region(PG_UP, (size_t)no * 4), oOI = hc.region(PG_UP, (size_t)no * 4),
                 oR = hc.region(PG_UP, (size_t)np * 4), oSel = hc.region(PG_UP, (size_t)nsel * 4),
                 oP = hc.region(PG_INOUT, (size_t)np * sizeof(pgorb_map_point)), oPD = hc.region(PG_INOUT, (size_t)np * 32),
                 oBest = hc.region(PG_DOWN, (size_t)nsel * 4), oSt = hc.region(PG_DOWN, (size_t)nsel * 4);
    int rc = hc.begin();
    if (rc) return rc;
    for (int f = 0; f < nkf; f++) {
        hc.put(oK, kps[f], (size_t)n[f] * kb, (size_t)f * cap * kb, (size_t)cap * kb);
        hc.put(oD, desc[f], (size_t)n[f] * 32, (size_t)f * cap * 32, (size_t)cap * 32);
    }
    hc.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oPose, pose, (size_t)nkf * sizeof(pgorb_kf_pose), 0, (size_t)nf * sizeof(pgorb_kf_pose));
    hc.put(oKB, kf_bad, nkf, 0, nf);
    hc.put(oB, point_bad, npoints, 0, np);
    hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oR, ref_obs, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oSel, select, (size_t)nsel * 4, 0, (size_t)nsel * 4);
    hc.put(oP, points, (size_t)npoints * sizeof(pgorb_map_point), 0, (size_t)np * sizeof(pgorb_map_point));
    hc.put(oPD, point_desc, (size_t)npoints * 32, 0, (size_t)np * 32);
    if ((rc = hc.run([&] {
            return pgorb_refresh_map_points_batch_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev(oD), hc.dev<int32_t>(oN), nkf, cap,
                                                         hc.dev<pgorb_kf_pose>(oPose), hc.dev(oKB), npoints, hc.dev<pgorb_map_point>(oP),
                                                         hc.dev(oPD), hc.dev(oB), hc.dev<int32_t>(oOS), hc.dev<int32_t>(oOF), hc.dev<int32_t>(oOI),
                                                         nobs, hc.dev<int32_t>(oR), nsel, select ? hc.dev<int32_t>(oSel) : nullptr, what,
                                                         hc.dev<int32_t>(oBest), hc.dev<int32_t>(oSt), nullptr); }))) return rc;
    memcpy(points, hc.host(oP), (size_t)npoints * sizeof(pgorb_map_point));
    memcpy(point_desc, hc.host(oPD), (size_t)npoints * 32);
    memcpy(status, hc.host(oSt), (size_t)nsel * 4);
    if (best_obs) memcpy(best_obs, hc.host(oBest), (size_t)nsel * 4);
    int changed = 0;
    for (int q = 0; q < nsel; q++) changed += status[q] > 0;
    return changed;
}

}  // extern "C"
