// window_match.hip -- the grid-window matchers on gfx950: SearchForInitialization and the three SearchByProjection forms.
//
// Restates (thirdparty/orb-slam2):
//   Frame::GetFeaturesInArea                  src/Frame.cc:331-384
//   ORBmatcher::SearchForInitialization       src/ORBmatcher.cc:407-522
//   ORBmatcher::SearchByProjection            src/ORBmatcher.cc:46-131 (local map points), 1355-1474 (last frame), 1476-1603 (key frame)
//   ORBmatcher::ComputeThreeMaxima            src/ORBmatcher.cc:1605-1646 (match_common.h)
//   MapPoint::PredictScale                    src/MapPoint.cc:516-531
//
// SearchForInitialization is sequential over F1's keypoints by construction: whether candidate i2 is
// considered depends on vMatchedDistance[i2], which earlier keypoints wrote (:445-446, :469).
// What does NOT depend on that order is the expensive part: which keypoints of F2 lie in the
// window of vbPrevMatched[i1] (it is only updated after the loop, :516-519) and their Hamming
// distances.  So the work is split:
//   k_sfi_candidates   one wave per (pair, F1 keypoint), all in parallel: lanes gather the grid
//       cells of the window (CSR ranges, wave prefix sum -> candidate list in the reference's
//       (column, row, insertion) order), filter by level and window (Frame.cc:354-376), evaluate
//       one 256-bit distance each and store the survivors in order as (distance << 16 | i2),
//       at most 64 per keypoint (more: the count says "overflow").
//   k_search_for_initialization   one wave per pair walks F1's keypoints that have candidates, in
//       order, with the stored lists prefetched two groups ahead: per keypoint one LDS gather of
//       vMatchedDistance, two wave reductions ("first minimum wins", :448-457: argmin on
//       distance << 16 | list position; second best over the other entries) and the update by one
//       lane -- no global round trip inside the chain (it was four per keypoint, 3.4 us each:
//       1.46 ms per pair; tools/next_tier_bench.py).  Overflowed keypoints are evaluated in place,
//       cell by cell.  The rotation histogram only needs (i1, the i2 it was matched to when pushed):
//       the bins are computed after the loop, in parallel.
// All per-pair state (vMatchedDistance, vnMatches21, vnMatches12) lives in LDS.
#include "proj_match.h"

// scratch layout for npairs x rowsPerPair rows; returns the bytes needed
static size_t pg_lists_layout(void* scratch, int npairs, int rowsPerPair, PgLists* L)
{
    const size_t rows = (size_t)npairs * rowsPerPair;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    uint8_t* b = (uint8_t*)scratch;
    L->poolTop = (int32_t*)(b + off); off += al((size_t)npairs * 4);
    L->fixed = (uint32_t*)(b + off); off += al(rows * LIST_K * 4);
    L->cnt = (uint16_t*)(b + off); off += al(rows * 2);
    L->ovf = (uint32_t*)(b + off); off += al(rows * 4);
    L->poolPerPair = (uint32_t)((size_t)rowsPerPair * LIST_POOL);
    L->pool = (uint32_t*)(b + off); off += al((size_t)npairs * L->poolPerPair * 4);
    return off;
}
// entry `pos` (any position) of a query row; chunk = 64 consecutive entries, one per lane
__device__ __forceinline__ uint32_t pg_list_chunk(const PgLists& L, int64_t row, int p, uint32_t ovf, int ch, int lane)
{
    return ch == 0 ? L.fixed[row * LIST_K + lane] : L.pool[(size_t)p * L.poolPerPair + ovf + (uint32_t)(ch - 1) * 64u + (uint32_t)lane];
}
// Pass A, the tail of a query's wave: `total` survivors are about to be written.  Reserves pool space when they do not fit the
// fixed slots; returns the pool offset (wave-uniform) and sets `over` when the pair's pool is full.
__device__ __forceinline__ uint32_t pg_list_reserve(const PgLists& L, int p, int total, int lane, bool& over)
{
    over = false;
    if (total <= LIST_K) return 0u;
    const int need = (total - LIST_K + 63) & ~63;
    int base = 0;
    if (lane == 0) base = atomicAdd(&L.poolTop[p], need);
    base = __builtin_amdgcn_readfirstlane(base);
    over = (uint32_t)base + (uint32_t)need > L.poolPerPair;
    return (uint32_t)base;
}

// Phase 1: candidate lists.  Workgroup = 4 waves = 4 consecutive F1 keypoints of pair blockIdx.y.
__global__ __launch_bounds__(256) void k_sfi_candidates(
    const pgorb_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc, const int32_t* __restrict__ nper,
    int cap, const int32_t* __restrict__ gstart, const int32_t* __restrict__ gidx,
    const int32_t* __restrict__ pairF1, const int32_t* __restrict__ pairF2,
    float minX, float minY, float invW, float invH, const float* __restrict__ prevMatched, int windowSize, PgLists Ls)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, p = blockIdx.y;
    const int i1 = blockIdx.x * 4 + wv;
    const int f1 = pairF1[p], f2 = pairF2[p];
    const int n1 = min(nper[f1], cap);
    if (i1 >= n1) return;
    const int64_t row = (int64_t)p * cap + i1;
    uint16_t* cntOut = Ls.cnt + row;
    const pgorb_keypoint kp1 = kps[(int64_t)f1 * cap + i1];
    int cx0, cx1, cy0, cy1;
    const float x = prevMatched[((int64_t)p * cap + i1) * 2], y = prevMatched[((int64_t)p * cap + i1) * 2 + 1];
    const float r = (float)windowSize;
    if (kp1.octave > 0 || !sfi_window(x, y, r, minX, minY, invW, invH, cx0, cx1, cy0, cy1)) {        // :424-426
        if (lane == 0) *cntOut = 0;
        return;
    }
    const int level1 = kp1.octave;
    const pgorb_keypoint* K2 = kps + (int64_t)f2 * cap;
    const uint8_t* D2 = desc + (int64_t)f2 * cap * 32;
    const int32_t* start2 = gstart + (int64_t)f2 * (GRID_CELLS + 1);
    const int32_t* idx2 = gidx + (int64_t)f2 * cap;
    uint16_t* candList = reinterpret_cast<uint16_t*>(pg_sfi_smem) + (size_t)wv * cap;      // this wave's vIndices2 before filtering
    const int ncy = cy1 - cy0 + 1, T = (cx1 - cx0 + 1) * ncy;
    int M = 0;
    for (int base = 0; base < T; base += 64) {                  // window cells in (ix, iy) order, entries in insertion order
        const int t = base + lane;
        int s0 = 0, cnt = 0;
        if (t < T) {
            const int c = (cx0 + t / ncy) * GRID_ROWS + cy0 + t % ncy;
            s0 = start2[c]; cnt = start2[c + 1] - s0;
        }
        const int incl = wave_incl_scan(cnt, lane);
        const int off = M + incl - cnt;
        for (int j = 0; j < cnt; j++) candList[off + j] = (uint16_t)idx2[s0 + j];
        M += __builtin_amdgcn_readlane(incl, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint4 q0 = reinterpret_cast<const uint4*>(desc + ((int64_t)f1 * cap + i1) * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(desc + ((int64_t)f1 * cap + i1) * 32)[1];
    // bCheckLevels is true for minLevel = maxLevel = 0 (Frame.cc:354): octave must equal level1
    auto survives = [&](int k, int& i2) {
        i2 = candList[k];
        const pgorb_keypoint kp2 = K2[i2];
        return kp2.octave == level1 && fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r;
    };
    // survivors beyond the fixed slots go to the pair's pool, reserved in one piece the moment the 65th survivor turns up -- for what
    // is left of the window's M keypoints, an upper bound (counting the survivors first cost a second pass over the keypoints, and
    // reserving for every query with M > 64 an atomic per query on the pair's counter: + 25 % / + 100 % on the whole matcher)
    int total = 0;
    bool over = false, reserved = false;
    uint32_t ovf = 0;
    uint32_t* out = Ls.fixed + row * LIST_K;
    uint32_t* outPool = Ls.pool + (size_t)p * Ls.poolPerPair;
    for (int base = 0; base < M; base += 64) {
        const int k = base + lane;
        int i2 = 0;
        const bool ok = k < M && survives(k, i2);
        const uint32_t e = ok ? (((uint32_t)sfi_distance(q0, q1, D2 + (int64_t)i2 * 32) << 16) | (uint32_t)i2) : 0u;
        const unsigned long long m = __ballot(ok);
        const int pos = total + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        total += __popcll(m);
        if (total > LIST_K && !reserved) { ovf = pg_list_reserve(Ls, p, LIST_K + (M - base), lane, over); reserved = true; }     // (wave-uniform)
        if (ok) { if (pos < LIST_K) out[pos] = e; else if (!over) outPool[ovf + (uint32_t)(pos - LIST_K)] = e; }
    }
    if (lane == 0) { *cntOut = (uint16_t)(over ? LIST_OVER : total); Ls.ovf[row] = ovf; }
}

// A keypoint of F1 with more than SFI_K candidates in its window (rare: every keypoint of a dense patch within 100 px):
// distances and the vMatchedDistance filter evaluated in place, cell by cell in the reference's (column, row, insertion)
// order.  Out: smallest (distance << 16 | running position), the second-smallest distance, the winner's i2.
// (results by value: reference parameters of a non-inlined function live in scratch memory, and the common path paid for it)
__device__ __noinline__ uint3 sfi_eval_in_place(const pgorb_keypoint kp1, float x, float y, float r, float minX, float minY, float invW,
                                                float invH, const uint8_t* d1, const pgorb_keypoint* K2, const uint8_t* D2,
                                                const int32_t* start2, const int32_t* idx2, const uint16_t* matchedDist, int lane)
{
    int cx0, cx1, cy0, cy1;
    sfi_window(x, y, r, minX, minY, invW, invH, cx0, cx1, cy0, cy1);          // (true: phase 1 got here)
    const uint4 q0 = reinterpret_cast<const uint4*>(d1)[0], q1 = reinterpret_cast<const uint4*>(d1)[1];
    unsigned b1key = 0xFFFFFFFFu, b1idx = 0; int b2 = 0x7fffffff; int posBase = 0;
    for (int ix = cx0; ix <= cx1; ix++)
        for (int iy = cy0; iy <= cy1; iy++) {
            const int c = ix * GRID_ROWS + iy, s0 = start2[c], cnt = start2[c + 1] - s0;
            for (int k = lane; k < cnt; k += 64) {
                const int i2 = idx2[s0 + k];
                const pgorb_keypoint kp2 = K2[i2];
                const float distx = __fsub_rn(kp2.x, x), disty = __fsub_rn(kp2.y, y);
                if (kp2.octave != kp1.octave || !(fabsf(distx) < r && fabsf(disty) < r)) continue;
                const int dist = sfi_distance(q0, q1, D2 + (int64_t)i2 * 32);
                if ((int)matchedDist[i2] <= dist) continue;
                const unsigned key = ((unsigned)dist << 16) | (unsigned)(posBase + k);     // posBase + k < cap < 2^16
                if (key < b1key) { if (b1key != 0xFFFFFFFFu) b2 = min(b2, (int)(b1key >> 16)); b1key = key; b1idx = (unsigned)i2; }
                else b2 = min(b2, dist);
            }
            posBase += cnt;
        }
    const unsigned wkey = wave_min_u32(b1key);
    if (wkey == 0xFFFFFFFFu) return make_uint3(wkey, 0x7fffffffu, 0u);
    const unsigned long long who = __ballot(b1key == wkey);
    const int bestIdx2 = __shfl((int)b1idx, __ffsll((long long)who) - 1);
    const unsigned mine = (b1key == wkey) ? (unsigned)b2 : (b1key == 0xFFFFFFFFu ? 0x7fffffffu : (b1key >> 16));
    return make_uint3(wkey, wave_min_u32(min(mine, (unsigned)b2)), (unsigned)bestIdx2);
}

// The long forms of a keypoint's evaluation in the sequential pass, out of line: a list longer than the fixed slots (chunk 0 = the
// prefetched `e0`, the rest 64 entries at a time from the pair's pool), or -- the pair's pool was full -- the evaluation in place.
// Out: smallest (distance << 16 | position), the second-smallest distance (0x7fffffff: none), the winner's i2.
__device__ __noinline__ uint3 sfi_eval_long(int count, uint32_t e0, const uint32_t* poolRow, const pgorb_keypoint kp1, float x, float y, float r,
                                            float minX, float minY, float invW, float invH, const uint8_t* d1, const pgorb_keypoint* K2,
                                            const uint8_t* D2, const int32_t* start2, const int32_t* idx2, const uint16_t* matchedDist, int lane)
{
    if (count == (int)LIST_OVER) return sfi_eval_in_place(kp1, x, y, r, minX, minY, invW, invH, d1, K2, D2, start2, idx2, matchedDist, lane);
    unsigned wkey = 0xFFFFFFFFu, second = 0xFFFFFFFFu;
    int bestIdx2 = -1;
    for (int ch = 0; ch * 64 < count; ch++) {
        const uint32_t ee = ch == 0 ? e0 : poolRow[(uint32_t)(ch - 1) * 64u + (uint32_t)lane];
        const int i2 = (int)(ee & 0xFFFFu), dist = (int)(ee >> 16);
        const bool keep = ch * 64 + lane < count && !((int)matchedDist[i2] <= dist);       // :445-446
        const unsigned key = keep ? (((unsigned)dist << 16) | (unsigned)(ch * 64 + lane)) : 0xFFFFFFFFu;
        unsigned k1, k2;
        wave_min2_u32(key, k1, k2);
        if (k1 < wkey) { second = min(wkey, k2); wkey = k1; bestIdx2 = __builtin_amdgcn_readlane(i2, (int)(k1 & 63u)); }
        else second = min(second, k1);
    }
    return make_uint3(wkey, second == 0xFFFFFFFFu ? 0x7fffffffu : (second >> 16), (unsigned)bestIdx2);
}

#define SFI_G 8                  // keypoints per prefetch group
// Phase 2: the sequential pass, one wave per pair.  (Round 4 also built this pass as ROUNDS of independent keypoints -- the scheme
// k_search_by_projection runs below -- and measured it slower here: every listed keypoint of a pair is a level-0 keypoint with a
// 200-px window, the lists overlap heavily, and the conservative readiness rule left ~10 % of the keypoints per round: 1.33 ms per 127
// pairs of 4 000 features against 0.68 ms for this walk; profiles/r04_next_tier.txt.  The lists are variable length now: a dense
// window no longer falls back to the evaluation in place.)
__global__ __launch_bounds__(64) void k_search_for_initialization(
    const pgorb_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc, const int32_t* __restrict__ nper,
    int cap, const int32_t* __restrict__ gstart, const int32_t* __restrict__ gidx,
    const int32_t* __restrict__ pairF1, const int32_t* __restrict__ pairF2,
    float minX, float minY, float invW, float invH,
    float* __restrict__ prevMatched, int32_t* __restrict__ matches12out, int32_t* __restrict__ nmatchesOut,
    int windowSize, float nnratio, int checkOrientation, PgLists Ls)
{
    const int lane = threadIdx.x, p = blockIdx.x;
    const int f1 = pairF1[p], f2 = pairF2[p];
    const int n1 = min(nper[f1], cap);
    const pgorb_keypoint* K1 = kps + (int64_t)f1 * cap;
    const pgorb_keypoint* K2 = kps + (int64_t)f2 * cap;
    const uint8_t* D1 = desc + (int64_t)f1 * cap * 32;
    const uint8_t* D2 = desc + (int64_t)f2 * cap * 32;
    const int32_t* start2 = gstart + (int64_t)f2 * (GRID_CELLS + 1);
    const int32_t* idx2 = gidx + (int64_t)f2 * cap;
    float* prev = prevMatched + (int64_t)p * cap * 2;
    int32_t* m12out = matches12out + (int64_t)p * cap;
    const int64_t row0 = (int64_t)p * cap;
    const uint32_t* L = Ls.fixed + row0 * LIST_K;
    const uint16_t* LC = Ls.cnt + row0;

    uint16_t* matchedDist = reinterpret_cast<uint16_t*>(pg_sfi_smem);      // [cap] vMatchedDistance (0xFFFF = INT_MAX)
    int16_t* m21 = reinterpret_cast<int16_t*>(matchedDist + cap);          // [cap] vnMatches21
    int16_t* m12 = m21 + cap;                                              // [cap] vnMatches12
    int16_t* push2 = m12 + cap;                                            // [cap] i2 an i1 was matched to when it entered the histogram, or -1
    uint16_t* active = reinterpret_cast<uint16_t*>(push2 + cap);           // [cap] F1 keypoints with candidates, in order
    for (int i = lane; i < cap; i += 64) { matchedDist[i] = 0xFFFF; m21[i] = -1; m12[i] = -1; push2[i] = -1; }
    int nact = 0;
    for (int base = 0; base < n1; base += 512) {                             // (8 count loads in flight, not one round trip per 64 keypoints)
        uint16_t cv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int i = base + 64 * u + lane; cv[u] = i < n1 ? LC[i] : (uint16_t)0; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const bool on = cv[u] != 0;
            const unsigned long long m = __ballot(on);
            if (on) active[nact + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0))] = (uint16_t)(base + 64 * u + lane);
            nact += __popcll(m);
        }
    }
    __syncthreads();

    const float r = (float)windowSize;
    int nmatches = 0;
    // group g = active[g * SFI_G .. ): entry `lane` of each member's list and its count, loaded one group ahead
    uint32_t curE[SFI_G], nxtE[SFI_G]; int curC[SFI_G], nxtC[SFI_G], curI[SFI_G], nxtI[SFI_G];
    auto load_group = [&](int g, uint32_t (&E)[SFI_G], int (&Cn)[SFI_G], int (&I)[SFI_G]) {
#pragma unroll
        for (int j = 0; j < SFI_G; j++) {
            const int a = g * SFI_G + j;
            I[j] = -1; Cn[j] = 0; E[j] = 0;
            if (a < nact) {
                const int i1 = active[a];
                I[j] = i1; Cn[j] = LC[i1];
                E[j] = L[(int64_t)i1 * SFI_K + lane];                        // (all 64 slots: no wait for the count; slots past it are masked below)
            }
        }
    };
    const int ngroups = (nact + SFI_G - 1) / SFI_G;
    if (ngroups) load_group(0, curE, curC, curI);
    for (int g = 0; g < ngroups; g++) {
        if (g + 1 < ngroups) load_group(g + 1, nxtE, nxtC, nxtI);
#pragma unroll
        for (int j = 0; j < SFI_G; j++) {
            const int i1 = curI[j];
            if (i1 < 0) break;                                              // (wave-uniform)
            unsigned wkey; int bestIdx2 = -1; unsigned second;
            if (curC[j] <= LIST_K) {
                // the common case, straight: the whole list is the prefetched chunk
                const int i2 = (int)(curE[j] & 0xFFFFu), dist = (int)(curE[j] >> 16);
                const bool keep = lane < curC[j] && !((int)matchedDist[i2] <= dist);       // :445-446
                const unsigned key = keep ? (((unsigned)dist << 16) | (unsigned)lane) : 0xFFFFFFFFu;
                wave_min2_u32(key, wkey, second);                           // smallest key, and the smallest of the others
                if (wkey == 0xFFFFFFFFu) continue;
                bestIdx2 = __builtin_amdgcn_readlane(i2, (int)(wkey & 0xFFFFu));
                second = (second == 0xFFFFFFFFu) ? 0x7fffffffu : (second >> 16);
            } else {
                // a dense window (the list continues in the pair's pool) or a pair whose pool is full (evaluation in place): out of line, so
                // that the eight unrolled copies of this body stay small -- inlined, the sequential wave lost 20 % to instruction fetch
                const uint3 ev = sfi_eval_long(curC[j], curE[j], Ls.pool + (size_t)p * Ls.poolPerPair + Ls.ovf[row0 + i1], K1[i1], prev[2 * i1], prev[2 * i1 + 1], r,
                                               minX, minY, invW, invH, D1 + (int64_t)i1 * 32, K2, D2, start2, idx2, matchedDist, lane);
                wkey = ev.x; second = ev.y; bestIdx2 = (int)ev.z;
                if (wkey == 0xFFFFFFFFu) continue;
            }
            const int bestDist = (int)(wkey >> 16);
            const float bestDist2 = (second >= 0x7fffffffu) ? 2147483648.0f : (float)(int)second;   // (float)INT_MAX
            if (bestDist <= TH_LOW && (float)bestDist < __fmul_rn(bestDist2, nnratio)) {            // :460-462
                const int old = m21[bestIdx2];
                if (old >= 0) nmatches--;                                    // :464-468
                nmatches++;
                if (lane == 0) {
                    if (old >= 0) m12[old] = -1;
                    m12[i1] = (int16_t)bestIdx2;
                    m21[bestIdx2] = (int16_t)i1;
                    matchedDist[bestIdx2] = (uint16_t)bestDist;
                    push2[i1] = (int16_t)bestIdx2;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
#pragma unroll
        for (int j = 0; j < SFI_G; j++) { curE[j] = nxtE[j]; curC[j] = nxtC[j]; curI[j] = nxtI[j]; }
    }
    __syncthreads();
    if (checkOrientation) {
        // histogram sizes = number of pushes per bin (a displaced i1 stays in its list, :481); the bin of a push is
        // a function of the two keypoints' angles (:473-483)
        int8_t* rotBin = reinterpret_cast<int8_t*>(active);                  // [n1] (the active list is done)
        int* hist = reinterpret_cast<int*>(pg_sfi_smem + (((size_t)cap * 10 + 3) & ~(size_t)3));      // [32] behind the arrays
        if (lane < 32) hist[lane] = 0;
        __syncthreads();
        for (int base = 0; base < n1; base += 256) {                         // (the angle loads of 4 x 64 keypoints in flight)
            int i2v[4]; float a1[4], a2[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = base + 64 * u + lane;
                i2v[u] = i < n1 ? (int)push2[i] : -1;
                a1[u] = 0.f; a2[u] = 0.f;
                if (i2v[u] >= 0) { a1[u] = K1[i].angle; a2[u] = K2[i2v[u]].angle; }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = base + 64 * u + lane;
                int bin = -1;
                if (i2v[u] >= 0) {
                    bin = pg_rot_bin(a1[u], a2[u]);
                    atomicAdd(&hist[bin], 1);
                }
                if (i < n1) rotBin[i] = (int8_t)bin;
            }
        }
        __syncthreads();
        const int h = lane < HISTO_LENGTH ? hist[lane] : 0;                  // lane b < 30 holds the size of bin b
        int ind1, ind2, ind3;
        pg_three_maxima([&](int i) { return __shfl(h, i); }, ind1, ind2, ind3);     // (:1605-1646)
        int removed = 0;
        for (int i = lane; i < n1; i += 64) {
            const int b = rotBin[i];
            if (b >= 0 && b != ind1 && b != ind2 && b != ind3 && m12[i] >= 0) { m12[i] = -1; removed++; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) removed += __shfl_xor(removed, d);
        nmatches -= removed;
        __syncthreads();
    }
    for (int base = 0; base < n1; base += 256) {                             // :516-519
        int mv[4]; float2 xy[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = base + 64 * u + lane;
            mv[u] = i < n1 ? (int)m12[i] : -1;
            xy[u] = make_float2(0.f, 0.f);
            if (mv[u] >= 0) xy[u] = *reinterpret_cast<const float2*>(&K2[mv[u]].x);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = base + 64 * u + lane;
            if (i < n1) m12out[i] = mv[u];
            if (mv[u] >= 0) *reinterpret_cast<float2*>(prev + 2 * i) = xy[u];
        }
    }
    if (lane == 0) nmatchesOut[p] = nmatches;
}

#ifndef RR_T
#define RR_T 1024               // threads of the rounds workgroup (one per pair); 512 in a developer build: tools/experiments/r4_rr_threads.sh
#endif
#define RR_W (RR_T / 64)
// ---- SearchByProjection (local map points / last frame), src/ORBmatcher.cc:46-131, 1355-1474 ----
// One wave per frame; queries in order.  mode 0: best + second with the same-level ratio test
// (:83-125); mode 1: best only + rotation histogram (:1390-1469).
// Batch layout (round 3): pair p = blockIdx.x matches its nq[p] queries against frame pairFrame[p] of an extract batch
// (keypoints / descriptors `cap` apart, grids (GRID_CELLS + 1) / cap apart); query arrays are [npairs][qcap].  The search
// radius and the level window of a query are derived here from what the caller holds (predicted level + viewing cosine,
// or the last frame's octave) exactly as the reference does, so the host never touches the queries.
// Round 3, two passes like SearchForInitialization: the candidates of a query and their distances do not depend on the
// assignments made so far (only `taken` does), so pass A computes them for every query of every pair in parallel and
// pass B -- one wave per pair, the reference's order -- only filters the stored candidates by `taken` and picks.
#define PROJ_K LIST_K            // candidates in a query's fixed slots; the rest of its list is in the pair's pool (PgLists)

// GetFeaturesInArea's window and the level range of query q; false = the reference skips the query
__device__ __forceinline__ bool proj_query(const PgProjBatch& B, int64_t qi, int mode, float minX, float minY, float invW, float invH,
                                           float& x, float& y, float& r, int& minLevel, int& maxLevel, int& cx0, int& cx1, int& cy0, int& cy1)
{
    if (!B.valid[qi]) return false;
    x = B.x[qi]; y = B.y[qi];
    int lvl;
    if (mode == 2) {
        // ORBmatcher.cc:1497-1531: not already found, projection inside the image bounds, depth inside the point's scale
        // invariance range, level from MapPoint::PredictScale
        if (B.found[qi]) return false;
        if (x < minX || x > B.maxX || y < minY || y > B.maxY) return false;          // :1512-1515
        // minDist / maxDist are mfMinDistance / mfMaxDistance: the depth test takes GetMin/MaxDistanceInvariance() =
        // 0.8f*mfMinDistance / 1.2f*mfMaxDistance (:1519-1526, MapPoint.cc:390-400), PredictScale the plain mfMaxDistance (MapPoint.cc:521)
        const float d3 = B.dist3d[qi], dmax = B.maxDist[qi];
        if (d3 < __fmul_rn(0.8f, B.minDist[qi]) || d3 > __fmul_rn(1.2f, dmax)) return false;
        lvl = pg_predict_scale(dmax, d3, B.logSf, B.nlevels);
    } else {
        lvl = B.level[qi];
        if (lvl < 0 || lvl >= B.nlevels) return false;
    }
    if (mode == 2) {
        r = __fmul_rn(B.th, B.sf[lvl]);                               // th * CurrentFrame.mvScaleFactors[nPredictedLevel] (:1531)
        minLevel = lvl - 1; maxLevel = lvl + 1;                       // :1533
    } else if (mode == 0) {
        r = ((double)B.aux[qi] > 0.998) ? 2.5f : 4.0f;                // RadiusByViewingCos (:133-139)
        if (B.th != 1.0f) r = __fmul_rn(r, B.th);                     // bFactor (:50, :65-66)
        r = __fmul_rn(r, B.sf[lvl]);                                  // r * F.mvScaleFactors[nPredictedLevel] (:69)
        minLevel = lvl - 1; maxLevel = lvl;                           // :69-70
    } else {
        r = __fmul_rn(B.th, B.sf[lvl]);                               // th * CurrentFrame.mvScaleFactors[nLastOctave] (:1383)
        minLevel = lvl - 1; maxLevel = lvl + 1;                       // :1392 (mono: neither forward nor backward)
    }
    return sfi_window(x, y, r, minX, minY, invW, invH, cx0, cx1, cy0, cy1);   // Frame.cc:336-350
}

// entry of a stored candidate: distance << 23 | rotation bin << 18 | octave << 14 | keypoint index
__device__ __forceinline__ uint32_t proj_entry(int dist, int bin, int octave, int i2)
{
    return ((uint32_t)dist << 23) | ((uint32_t)(bin & 31) << 18) | ((uint32_t)(octave & 15) << 14) | (uint32_t)i2;
}

// Pass A: workgroup = 4 waves = 4 consecutive queries of pair blockIdx.y
__global__ __launch_bounds__(256) void k_proj_candidates(PgProjBatch B, float minX, float minY, float invW, float invH, int mode, PgLists Ls)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, p = blockIdx.y;
    const int q = blockIdx.x * 4 + wv;
    const int nq = min(B.nq[p], B.qcap);
    if (q >= nq) return;
    const int frame = B.pairFrame ? B.pairFrame[p] : p, cap = B.cap;
    const int64_t qi = (int64_t)p * B.qcap + q;
    uint16_t* cntOut = Ls.cnt + qi;
    float x, y, r; int minLevel, maxLevel, cx0, cx1, cy0, cy1;
    if (!proj_query(B, qi, mode, minX, minY, invW, invH, x, y, r, minLevel, maxLevel, cx0, cx1, cy0, cy1)) {
        if (lane == 0) *cntOut = 0;
        return;
    }
    const pgorb_keypoint* __restrict__ K = B.K + (int64_t)frame * cap;
    const uint8_t* __restrict__ D = B.D + (int64_t)frame * cap * 32;
    const int32_t* __restrict__ gstart = B.gstart + (int64_t)frame * (GRID_CELLS + 1);
    const int32_t* __restrict__ gidx = B.gidx + (int64_t)frame * cap;
    uint16_t* candList = reinterpret_cast<uint16_t*>(pg_sfi_smem) + (size_t)wv * cap;
    const int ncy = cy1 - cy0 + 1, T = (cx1 - cx0 + 1) * ncy;
    int M = 0;
    for (int base = 0; base < T; base += 64) {                  // window cells in (ix, iy) order, entries in insertion order
        const int t = base + lane;
        int s0 = 0, cnt = 0;
        if (t < T) {
            const int c = (cx0 + t / ncy) * GRID_ROWS + cy0 + t % ncy;
            s0 = gstart[c]; cnt = gstart[c + 1] - s0;
        }
        const int incl = wave_incl_scan(cnt, lane);
        const int off = M + incl - cnt;
        for (int j = 0; j < cnt; j++) candList[off + j] = (uint16_t)gidx[s0 + j];
        M += __builtin_amdgcn_readlane(incl, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const uint4 q0 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[1];
    const float qangle = mode != 0 ? B.aux[qi] : 0.f;
    auto survives = [&](int k, int& i2, pgorb_keypoint& kp2) {
        i2 = candList[k];
        kp2 = K[i2];
        if (bCheckLevels && (kp2.octave < minLevel || (maxLevel >= 0 && kp2.octave > maxLevel))) return false;
        return fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r;
    };
    // (survivors beyond the fixed slots: the pair's pool, reserved when the 65th turns up -- see k_sfi_candidates)
    int total = 0;
    bool over = false, reserved = false;
    uint32_t ovf = 0;
    uint32_t* out = Ls.fixed + qi * LIST_K;
    uint32_t* outPool = Ls.pool + (size_t)p * Ls.poolPerPair;
    for (int base = 0; base < M; base += 64) {
        const int k = base + lane;
        int i2 = 0; pgorb_keypoint kp2;
        const bool ok = k < M && survives(k, i2, kp2);
        const uint32_t e = ok ? proj_entry(sfi_distance(q0, q1, D + (int64_t)i2 * 32), mode != 0 ? pg_rot_bin(qangle, kp2.angle) : 0, kp2.octave, i2) : 0u;
        const unsigned long long m = __ballot(ok);
        const int pos = total + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        total += __popcll(m);
        if (total > LIST_K && !reserved) { ovf = pg_list_reserve(Ls, p, LIST_K + (M - base), lane, over); reserved = true; }     // (wave-uniform)
        if (ok) { if (pos < LIST_K) out[pos] = e; else if (!over) outPool[ovf + (uint32_t)(pos - LIST_K)] = e; }
    }
    if (lane == 0) { *cntOut = (uint16_t)(over ? LIST_OVER : total); Ls.ovf[qi] = ovf; }
}

// a query with more than PROJ_K candidates: the whole evaluation in place, in the reference's order (the round-2 form of the
// kernel); returns the best two entries, their keys' distances in the entry's distance field
__device__ __noinline__ uint2 proj_eval_in_place(const PgProjBatch B, int64_t qi, int frame, int mode, float minX, float minY, float invW,
                                                 float invH, const uint8_t* taken, int lane)
{
    float x, y, r; int minLevel, maxLevel, cx0, cx1, cy0, cy1;
    proj_query(B, qi, mode, minX, minY, invW, invH, x, y, r, minLevel, maxLevel, cx0, cx1, cy0, cy1);      // (true: pass A got here)
    const int cap = B.cap;
    const pgorb_keypoint* K = B.K + (int64_t)frame * cap;
    const uint8_t* D = B.D + (int64_t)frame * cap * 32;
    const int32_t* gstart = B.gstart + (int64_t)frame * (GRID_CELLS + 1);
    const int32_t* gidx = B.gidx + (int64_t)frame * cap;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const uint4 q0 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[1];
    const float qangle = mode != 0 ? B.aux[qi] : 0.f;
    unsigned long long b1 = ~0ull, b2 = ~0ull;              // (distance << 48 | scan position << 32 | entry): the lane's two smallest
    int posBase = 0;
    for (int ix = cx0; ix <= cx1; ix++)
        for (int iy = cy0; iy <= cy1; iy++) {
            const int c = ix * GRID_ROWS + iy, s0 = gstart[c], cnt = gstart[c + 1] - s0;
            for (int k = lane; k < cnt; k += 64) {
                const int i2 = gidx[s0 + k];
                const pgorb_keypoint kp2 = K[i2];
                if (bCheckLevels && (kp2.octave < minLevel || (maxLevel >= 0 && kp2.octave > maxLevel))) continue;
                if (!(fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r)) continue;
                if (taken[i2]) continue;
                const int dist = sfi_distance(q0, q1, D + (int64_t)i2 * 32);
                const unsigned long long key = ((unsigned long long)dist << 48) | ((unsigned long long)(posBase + k) << 32) |
                                               proj_entry(dist, mode != 0 ? pg_rot_bin(qangle, kp2.angle) : 0, kp2.octave, i2);
                if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
            }
            posBase += cnt;
        }
    // the wave's two smallest keys
    unsigned long long w1 = b1;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(w1, d); w1 = o < w1 ? o : w1; }
    unsigned long long mine = (b1 == w1) ? b2 : b1, w2 = mine;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(w2, d); w2 = o < w2 ? o : w2; }
    return make_uint2(w1 == ~0ull ? 0xFFFFFFFFu : (uint32_t)w1, w2 == ~0ull ? 0xFFFFFFFFu : (uint32_t)w2);
}

// Pass B (round 4): the queries of a pair in the reference's ORDER without its sequence.  What query q decides depends on earlier
// queries only through the "holds a point" state of the keypoints in q's own list (:79-81 / :1397-1399 / :1542-1543), and a query
// only ever writes that state for the ONE keypoint it takes, a candidate of its list within the acceptance threshold (TH_HIGH, or
// ORBdist in the key-frame form): its "takeable" candidates.  So q can be decided as soon as no UNDECIDED earlier query has a takeable
// candidate in q's list -- and (mode 0 only: the second best of its ratio test reads candidates beyond TH_HIGH too; the best-only
// forms decide the same either way) q must not take a keypoint an undecided earlier query still has to read -- "deterministic reservations":
//   round:  minq[i]   = the smallest undecided query with keypoint i among its takeable candidates     (LDS atomicMin, all undecided in parallel)
//           minAny[i] = the smallest undecided query with keypoint i anywhere in its list              (mode 0)
//           q is ready  <=>  minq[i] >= q for every i in q's list (and minAny[i] >= q for every takeable i of it);
//           ready queries decide from the state as it is (reads only), then, behind a barrier, apply their decisions
//           (two ready queries never take the same keypoint: the later one would not be ready).
// The smallest undecided query is always ready, so the rounds end; map points project to different places, a query conflicts with a
// handful of neighbours, and about half of the undecided ones fall in every round.  One workgroup of 16 waves per pair, a wave per
// query and round, four queries' lists in flight per wave.  (Rounds 2-3: one wave walked the ~1 500-3 000 queries of a pair one after
// the other, ~0.4 us each: 1.64 ms for a single 3 200-point call against 0.58 ms on one CPU core; now 0.49 ms, and 127 pairs in
// 0.52 ms instead of 1.04.)  A query whose list did not fit the pool (LIST_OVER) waits until it is the smallest undecided one, holds
// back everything behind it, and is evaluated in place.  The rule against the plain sequence on random lists, without a GPU:
// tests/test_host_logic.py.  (SearchForInitialization keeps its sequential wave: see there.)
__global__ __launch_bounds__(RR_T) void k_search_by_projection(
    PgProjBatch B, float minX, float minY, float invW, float invH, int mode, float nnratio, int checkOrientation,
    PgLists Ls, int32_t* __restrict__ assignedOut, int32_t* __restrict__ nmatchesOut)
{
    const int p = blockIdx.x, frame = B.pairFrame ? B.pairFrame[p] : p;
    const int cap = B.cap, n = min(B.n[frame], cap), nq = min(B.nq[p], B.qcap);
    const uint8_t* kpHasPoint = B.kpHasPoint ? B.kpHasPoint + (int64_t)p * cap : nullptr;
    const int64_t qo = (int64_t)p * B.qcap;
    assignedOut += (int64_t)p * cap; nmatchesOut += p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int thTake = mode == 2 ? B.orbDist : TH_HIGH;
    // state in LDS: taken[i] = keypoint i holds a point (with observations, modes 0 / 1) before or by this call; asg[i] = query
    // assigned to keypoint i by this call; per query: list length, decision (keypoint, rotation bin), state
    uint32_t* minq = reinterpret_cast<uint32_t*>(pg_sfi_smem);            // [cap] smallest undecided query that may TAKE keypoint i
    uint32_t* minAny = minq + cap;                                        // [cap] smallest undecided query that LISTS keypoint i (mode 0: the second best of the ratio test)
    int32_t* asg = reinterpret_cast<int32_t*>(minAny + cap);               // [cap]
    int* ctrl = asg + cap;                                                // [8] counters, [8..40) the rotation histogram
    uint16_t* listA = reinterpret_cast<uint16_t*>(ctrl + 40);             // [qcap] undecided queries (two buffers)
    uint16_t* listB = listA + B.qcap;
    uint16_t* cntL = listB + B.qcap;                                      // [qcap]
    uint16_t* qBest = cntL + B.qcap;                                      // [qcap] keypoint the query takes
    int8_t* rotBin = reinterpret_cast<int8_t*>(qBest + B.qcap);           // [qcap] rotation bin of an accepted query (modes 1 / 2), or -1
    uint8_t* done = reinterpret_cast<uint8_t*>(rotBin + B.qcap);          // [qcap] 0 undecided, 1 decided to take qBest (to be applied), 2 finished
    uint8_t* taken = done + B.qcap;                                       // [cap]
    for (int i = tid; i < cap; i += RR_T) { taken[i] = (kpHasPoint && i < n) ? (kpHasPoint[i] != 0) : 0; asg[i] = -1; }
    if (tid < 40) ctrl[tid] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += RR_T) {
        const uint16_t c = Ls.cnt[qo + i];
        cntL[i] = c; rotBin[i] = -1; done[i] = 0;
        if (c) listA[atomicAdd(&ctrl[0], 1)] = (uint16_t)i;
    }
    __syncthreads();
    uint16_t* cur = listA; uint16_t* nxt = listB;
    int curC = 0;
    while (true) {
        const int nun = ctrl[curC];
        if (nun == 0) break;
        for (int k = tid; k < cap; k += RR_T) { minq[k] = 0xFFFFFFFFu; minAny[k] = 0xFFFFFFFFu; }
        if (tid == 0) { ctrl[1 - curC] = 0; ctrl[3] = 0x7fffffff; ctrl[4] = 0x7fffffff; }
        __syncthreads();
        // ---- takeable candidates of every undecided query ----
        for (int u0 = wv * 4; u0 < nun; u0 += RR_W * 4) {
            int q[4], c[4]; uint32_t e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                q[j] = u0 + j < nun ? (int)cur[u0 + j] : -1;
                c[j] = q[j] >= 0 ? (int)cntL[q[j]] : 0;
                e[j] = (c[j] != (int)LIST_OVER && lane < min(c[j], LIST_K)) ? Ls.fixed[(qo + q[j]) * LIST_K + lane] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (q[j] < 0) break;
                if (lane == 0) atomicMin(&ctrl[4], q[j]);
                if (c[j] == (int)LIST_OVER) { if (lane == 0) atomicMin(&ctrl[3], q[j]); continue; }
                const uint32_t ovf = c[j] > LIST_K ? Ls.ovf[qo + q[j]] : 0u;
                for (int ch = 0; ch * 64 < c[j]; ch++) {
                    const uint32_t ee = ch == 0 ? e[j] : pg_list_chunk(Ls, qo + q[j], p, ovf, ch, lane);
                    if (ch * 64 + lane < c[j]) {
                        if (mode == 0) atomicMin(&minAny[ee & 0x3FFFu], (uint32_t)q[j]);
                        if ((int)(ee >> 23) <= thTake) atomicMin(&minq[ee & 0x3FFFu], (uint32_t)q[j]);
                    }
                }
            }
        }
        __syncthreads();
        const int minOver = ctrl[3], minAll = ctrl[4];
        // ---- ready queries decide ----
        for (int u0 = wv * 4; u0 < nun; u0 += RR_W * 4) {
            int q[4], c[4]; uint32_t e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                q[j] = u0 + j < nun ? (int)cur[u0 + j] : -1;
                c[j] = q[j] >= 0 ? (int)cntL[q[j]] : 0;
                e[j] = (c[j] != (int)LIST_OVER && lane < min(c[j], LIST_K)) ? Ls.fixed[(qo + q[j]) * LIST_K + lane] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int qq = q[j];
                if (qq < 0) break;
                const bool isOver = c[j] == (int)LIST_OVER;
                const uint32_t ovf = (!isOver && c[j] > LIST_K) ? Ls.ovf[qo + qq] : 0u;
                bool ready = isOver ? (qq == minAll) : (qq < minOver);
                if (ready && !isOver)
                    for (int ch = 0; ch * 64 < c[j]; ch++) {
                        const uint32_t ee = ch == 0 ? e[j] : pg_list_chunk(Ls, qo + qq, p, ovf, ch, lane);
                        // (mode 0 only: a query must not take a keypoint an undecided EARLIER query still has to read -- the second best of
                        //  its ratio test looks at candidates beyond TH_HIGH too; the best-only forms decide the same either way)
                        const bool blocked = minq[ee & 0x3FFFu] < (uint32_t)qq ||
                                             (mode == 0 && (int)(ee >> 23) <= thTake && minAny[ee & 0x3FFFu] < (uint32_t)qq);
                        if (__ballot(ch * 64 + lane < c[j] && blocked) != 0ull) { ready = false; break; }
                    }
                if (!ready) { if (lane == 0) nxt[atomicAdd(&ctrl[1 - curC], 1)] = (uint16_t)qq; continue; }
                // best and second best of the candidates that hold no point (:79-81 / :1397-1399 / :1542-1543); first minimum wins:
                // key = distance << 16 | position in the list
                uint32_t e1 = 0xFFFFFFFFu, e2 = 0xFFFFFFFFu;
                if (!isOver) {
                    unsigned w1 = 0xFFFFFFFFu, w2 = 0xFFFFFFFFu;
                    for (int ch = 0; ch * 64 < c[j]; ch++) {
                        const uint32_t ee = ch == 0 ? e[j] : pg_list_chunk(Ls, qo + qq, p, ovf, ch, lane);
                        const bool keep = ch * 64 + lane < c[j] && !taken[ee & 0x3FFFu];
                        const unsigned key = keep ? (((ee >> 23) << 16) | (unsigned)(ch * 64 + lane)) : 0xFFFFFFFFu;
                        unsigned k1, k2;
                        wave_min2_u32(key, k1, k2);
                        const uint32_t c1 = k1 == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readlane((int)ee, (int)(k1 & 63u));
                        const uint32_t c2 = k2 == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readlane((int)ee, (int)(k2 & 63u));
                        if (k1 < w1) {
                            if (w1 < k2) { w2 = w1; e2 = e1; } else { w2 = k2; e2 = c2; }
                            w1 = k1; e1 = c1;
                        } else if (k1 < w2) { w2 = k1; e2 = c1; }
                    }
                } else {
                    const uint2 ev = proj_eval_in_place(B, qo + qq, frame, mode, minX, minY, invW, invH, taken, lane);
                    e1 = ev.x; e2 = ev.y;
                }
                bool accept = false;
                int bin = -1, bestIdx = 0;
                if (e1 != 0xFFFFFFFFu && (int)(e1 >> 23) < 256) {                   // bestDist starts at 256 (:74 / :1390 / :1536)
                    const int bestDist = (int)(e1 >> 23);
                    bestIdx = (int)(e1 & 0x3FFFu);
                    if (mode == 0) {
                        const bool has2 = e2 != 0xFFFFFFFFu && (int)(e2 >> 23) < 256;
                        const int bestDist2 = has2 ? (int)(e2 >> 23) : 256;
                        const int bestLevel = (int)((e1 >> 14) & 15u), bestLevel2 = has2 ? (int)((e2 >> 14) & 15u) : -1;
                        if (bestDist <= TH_HIGH)                                    // :113-123
                            accept = !(bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2));
                    } else {
                        accept = bestDist <= thTake;                                // :1421 / :1554
                        if (accept && checkOrientation) bin = (int)((e1 >> 18) & 31u);     // :1426-1436 / :1559-1569 (computed in pass A)
                    }
                }
                if (lane == 0) {
                    if (accept) { qBest[qq] = (uint16_t)bestIdx; rotBin[qq] = (int8_t)bin; done[qq] = 1; }
                    else done[qq] = 2;
                }
            }
        }
        __syncthreads();
        // ---- apply: F.mvpMapPoints[bestIdx] = pMP (two queries of one round never take the same keypoint) ----
        for (int u = tid; u < nun; u += RR_T) {
            const int qq = cur[u];
            if (done[qq] != 1) continue;
            const int k = qBest[qq];
            asg[k] = qq;
            taken[k] = mode == 2 ? 1 : (B.hasObs[qo + qq] != 0);                  // (key-frame form: any point blocks, :1542-1543)
            atomicAdd(&ctrl[2], 1);
            done[qq] = 3;                                                           // accepted and applied
        }
        __syncthreads();
        uint16_t* t = cur; cur = nxt; nxt = t;
        curC = 1 - curC;
    }
    __syncthreads();
    if (mode != 0 && checkOrientation) {                       // :1443-1469 / :1575-1600
        int* hist = ctrl + 8;
        for (int i = tid; i < nq; i += RR_T) if (rotBin[i] >= 0) atomicAdd(&hist[rotBin[i]], 1);
        __syncthreads();
        int ind1, ind2, ind3;
        pg_three_maxima([&](int i) { return hist[i]; }, ind1, ind2, ind3);
        // rotHist[bin] holds bestIdx2 of every accepted query; every entry of a rejected bin resets
        // its keypoint to NULL and is counted out once (:1458-1465)
        int removed = 0;
        for (int i = tid; i < nq; i += RR_T) {
            const int bb = rotBin[i];
            if (bb >= 0 && bb != ind1 && bb != ind2 && bb != ind3) { asg[qBest[i]] = -1; removed++; }
        }
        if (removed) atomicSub(&ctrl[2], removed);
        __syncthreads();
    }
    for (int i = tid; i < cap; i += RR_T) assignedOut[i] = i < n ? asg[i] : -1;
    if (tid == 0) *nmatchesOut = ctrl[2];
}

// the candidate lists of npairs x rowsPerPair queries in the matchers' scratch arena, the pools empty
static int pg_lists_acquire(pgorb_ctx* c, int npairs, int rowsPerPair, hipStream_t stream, PgLists* L)
{
    void* scratch;
    const int rc = pg_ctx_scratch(c, pg_lists_layout(nullptr, npairs, rowsPerPair, L) + 256, stream, &scratch);
    if (rc) return rc;
    pg_lists_layout(scratch, npairs, rowsPerPair, L);
    if (hipMemsetAsync(L->poolTop, 0, (size_t)npairs * 4, stream) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    return 0;
}

int pg_proj_begin(pgorb_ctx* c, int cap, int qcap, int npairs, size_t extraBytes, hipStream_t stream, PgLists* Ls, void** extra)
{
    if (cap > 16000 || qcap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    if (!pg_raise_lds<k_search_by_projection>(c, pg_sbp_lds(cap, qcap)) ||
        !pg_raise_lds<k_proj_candidates>(c, (size_t)4 * cap * 2)) return pg_ctx_fail(c, PGORB_E_LIMIT, PG_SBP_LDS_MSG);
    const int rows = std::max(qcap, 1);
    const size_t lists = pg_lists_layout(nullptr, npairs, rows, Ls) + 256;
    void* scratch;
    const int rc = pg_ctx_scratch(c, lists + extraBytes, stream, &scratch);
    if (rc) return rc;
    pg_lists_layout(scratch, npairs, rows, Ls);
    if (extra) *extra = (uint8_t*)scratch + lists;
    if (hipMemsetAsync(Ls->poolTop, 0, (size_t)npairs * 4, stream) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    return 0;
}

int pg_proj_run(pgorb_ctx* c, PgProjBatch& B, int npairs, float min_x, float max_x, float min_y, float max_y, int mode, float nnratio,
                int check_orientation, const PgLists& Ls, int32_t* d_assigned, int32_t* d_nmatches, hipStream_t stream)
{
    B.nlevels = pgorb_levels(c); B.maxX = max_x; B.maxY = max_y;
    pgorb_scale_tables(c, B.sf, nullptr, nullptr, nullptr);
    const float invW = (float)GRID_COLS / (max_x - min_x), invH = (float)GRID_ROWS / (max_y - min_y);
    const int cap = B.cap, qcap = B.qcap;
    if (qcap) hipLaunchKernelGGL(k_proj_candidates, dim3((qcap + 3) / 4, npairs), dim3(256), (size_t)4 * cap * 2, stream, B, min_x, min_y, invW,
                                 invH, mode, Ls);
    hipLaunchKernelGGL(k_search_by_projection, dim3(npairs), dim3(RR_T), pg_sbp_lds(cap, qcap), stream, B, min_x, min_y, invW, invH, mode,
                       nnratio, check_orientation, Ls, d_assigned, d_nmatches);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_search_by_projection launch failed");
    return pg_ctx_scratch_done(c, stream);
}

static int pg_search_by_projection_batch(pgorb_ctx* c, int mode, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                         const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
                                         float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point, int qcap,
                                         const int32_t* d_nq, const uint8_t* d_valid, const float* d_x, const float* d_y, const int32_t* d_level,
                                         const float* d_aux, const uint8_t* d_qdesc, const uint8_t* d_qobs, float th, float nnratio,
                                         int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, hipStream_t stream,
                                         const PgProjKeyFrame* kf = nullptr)
{
    const bool m2 = mode == 2;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || npairs < 0 || qcap < 0 ||
        (npairs && (!d_nq || !d_assigned || !d_nmatches)) ||
        (npairs && qcap && (!d_valid || !d_x || !d_y || !d_aux || !d_qdesc || (!m2 && (!d_level || !d_qobs)))) ||
        (m2 && (!kf || (npairs && qcap && (!kf->found || !kf->dist3d || !kf->minDist || !kf->maxDist)) || !(kf->logSf > 0.0f))) ||
        !(max_x > min_x) || !(max_y > min_y))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_projection_*");
    if (cap > 16000 || qcap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
    if (!npairs) return 0;
    PgLists Ls;                                                                    // of every query of every pair
    const int rcs = pg_proj_begin(c, cap, qcap, npairs, 0, stream, &Ls, nullptr);
    if (rcs) return rcs;
    PgProjBatch B;
    B.K = d_kps; B.D = d_desc; B.n = d_n; B.cap = cap; B.gstart = d_grid_start; B.gidx = d_grid_idx; B.pairFrame = d_pair_frame;
    B.kpHasPoint = d_kp_has_point; B.qcap = qcap; B.nq = d_nq; B.valid = d_valid; B.x = d_x; B.y = d_y; B.level = d_level; B.aux = d_aux;
    B.desc = d_qdesc; B.hasObs = d_qobs; B.th = th;
    B.found = nullptr; B.dist3d = B.minDist = B.maxDist = nullptr; B.logSf = 1.0f; B.orbDist = TH_HIGH;
    if (m2) { B.found = kf->found; B.dist3d = kf->dist3d; B.minDist = kf->minDist; B.maxDist = kf->maxDist; B.logSf = kf->logSf; B.orbDist = kf->orbDist; }
    return pg_proj_run(c, B, npairs, min_x, max_x, min_y, max_y, mode, nnratio, check_orientation, Ls, d_assigned, d_nmatches, stream);
}

// single frame through host buffers: a one-pair batch
static int pg_search_by_projection_host(pgorb_ctx* c, int mode, const pgorb_keypoint* kps, const uint8_t* desc, int n,
                                        float min_x, float max_x, float min_y, float max_y, const uint8_t* kp_has_point,
                                        int nq, const uint8_t* valid, const float* qx, const float* qy, const int32_t* level,
                                        const float* aux, const uint8_t* qdesc, const uint8_t* qobs, float th, float nnratio,
                                        int check_orientation, int32_t* assigned, const PgProjKeyFrame* kf = nullptr)
{
    const bool m2 = mode == 2;
    if (n < 0 || nq < 0 || (n && (!kps || !desc || !assigned)) ||
        (nq && (!valid || !qx || !qy || !aux || !qdesc || (!m2 && (!level || !qobs)))) ||
        (m2 && (!kf || (nq && (!kf->found || !kf->dist3d || !kf->minDist || !kf->maxDist)))) ||
        !(max_x > min_x) || !(max_y > min_y))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_projection_*");
    for (int i = 0; i < n; i++) assigned[i] = -1;
    if (!n || !nq) return 0;
    if (n > 16000 || nq > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
    if (pg_sbp_lds(n, nq) > PG_SBP_LDS_MAX) return pg_ctx_fail(c, PGORB_E_LIMIT, PG_SBP_LDS_MSG);      // (before anything is staged)
    const size_t q4 = (size_t)nq * 4, k4 = m2 ? q4 : 0;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 8), oK = s.region(PG_UP, (size_t)n * sizeof(pgorb_keypoint)), oD = s.region(PG_UP, (size_t)n * 32),
                 oH = s.region(PG_UP, n), oV = s.region(PG_UP, nq), oX = s.region(PG_UP, q4), oY = s.region(PG_UP, q4), oL = s.region(PG_UP, q4),
                 oA = s.region(PG_UP, q4), oQD = s.region(PG_UP, (size_t)nq * 32), oO = s.region(PG_UP, nq), oF = s.region(PG_UP, m2 ? nq : 0),
                 oD3 = s.region(PG_UP, k4), oDmin = s.region(PG_UP, k4), oDmax = s.region(PG_UP, k4), oAs = s.region(PG_DOWN, (size_t)n * 4),
                 oR = s.region(PG_DOWN, 4), oGS = s.region(PG_DEV, (size_t)(GRID_CELLS + 1) * 4), oGI = s.region(PG_DEV, (size_t)n * 4);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t cnt[2] = {n, nq};
    s.put(oN, cnt, 8); s.put(oK, kps, (size_t)n * sizeof(pgorb_keypoint)); s.put(oD, desc, (size_t)n * 32); s.put(oH, kp_has_point, n);
    s.put(oV, valid, nq); s.put(oX, qx, q4); s.put(oY, qy, q4); s.put(oL, level, q4); s.put(oA, aux, q4);
    s.put(oQD, qdesc, (size_t)nq * 32); s.put(oO, qobs, nq);
    if (m2) { s.put(oF, kf->found, nq); s.put(oD3, kf->dist3d, q4); s.put(oDmin, kf->minDist, q4); s.put(oDmax, kf->maxDist, q4); }
    const PgProjKeyFrame dkf = {s.dev(oF), s.dev<float>(oD3), s.dev<float>(oDmin), s.dev<float>(oDmax), m2 ? kf->logSf : 1.0f, m2 ? kf->orbDist : 0};
    if ((rc = s.run([&] {
            int r = pgorb_frame_grid_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), 1, n, min_x, max_x, min_y, max_y,
                                                  s.dev<int32_t>(oGS), s.dev<int32_t>(oGI), nullptr);
            return r ? r : pg_search_by_projection_batch(c, mode, s.dev<pgorb_keypoint>(oK), s.dev(oD), s.dev<int32_t>(oN), n, s.dev<int32_t>(oGS),
                                                         s.dev<int32_t>(oGI), nullptr, 1, min_x, max_x, min_y, max_y, kp_has_point ? s.dev(oH) : nullptr,
                                                         nq, s.dev<int32_t>(oN) + 1, s.dev(oV), s.dev<float>(oX), s.dev<float>(oY), s.dev<int32_t>(oL),
                                                         s.dev<float>(oA), s.dev(oQD), s.dev(oO), th, nnratio, check_orientation, s.dev<int32_t>(oAs),
                                                         s.dev<int32_t>(oR), nullptr, m2 ? &dkf : nullptr); }))) return rc;
    memcpy(assigned, s.host(oAs), (size_t)n * 4);
    return *s.host<int32_t>(oR);
}

extern "C" {

int pgorb_search_for_initialization(pgorb_ctx* c, const pgorb_keypoint* kps1, const uint8_t* desc1, int n1,
                                    const pgorb_keypoint* kps2, const uint8_t* desc2, int n2,
                                    float min_x, float max_x, float min_y, float max_y, float* prev_matched,
                                    int32_t* matches12, int window_size, float nnratio, int check_orientation)
{
    if (!c) return PGORB_E_ARG;
    if (n1 < 0 || n2 < 0 || (n1 && (!kps1 || !desc1 || !prev_matched || !matches12)) || (n2 && (!kps2 || !desc2)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_for_initialization");
    if (n1 == 0) return 0;
    const int cap = std::max(n1, n2);
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");      // (before anything is staged)
    const size_t kb = sizeof(pgorb_keypoint);
    PgHostCall s(c);
    const size_t oMisc = s.region(PG_UP, 16), oK = s.region(PG_UP, (size_t)2 * cap * kb), oD = s.region(PG_UP, (size_t)2 * cap * 32),
                 oP = s.region(PG_INOUT, (size_t)cap * 8), oM = s.region(PG_DOWN, (size_t)cap * 4), oNm = s.region(PG_DOWN, 4),
                 oGS = s.region(PG_DEV, (size_t)2 * (GRID_CELLS + 1) * 4), oGI = s.region(PG_DEV, (size_t)2 * cap * 4);
    int rc = s.begin();
    if (rc) return rc;
    const int32_t misc[4] = {n1, n2, 0, 1};   // n[2], f1, f2
    s.put(oMisc, misc, sizeof(misc));
    s.put(oK, kps1, n1 * kb); s.put(oK, kps2, n2 * kb, cap * kb);
    s.put(oD, desc1, (size_t)n1 * 32); s.put(oD, desc2, (size_t)n2 * 32, (size_t)cap * 32);
    s.put(oP, prev_matched, (size_t)n1 * 8);
    pgorb_keypoint* dk = s.dev<pgorb_keypoint>(oK);
    int32_t* dmisc = s.dev<int32_t>(oMisc);
    if ((rc = s.run([&] {
            int r = pgorb_frame_grid_batch_device(c, dk, dmisc, 2, cap, min_x, max_x, min_y, max_y, s.dev<int32_t>(oGS), s.dev<int32_t>(oGI), nullptr);
            return r ? r : pgorb_search_for_initialization_batch_device(c, dk, s.dev(oD), dmisc, cap, s.dev<int32_t>(oGS), s.dev<int32_t>(oGI), dmisc + 2,
                                                                        dmisc + 3, 1, min_x, max_x, min_y, max_y, s.dev<float>(oP), s.dev<int32_t>(oM),
                                                                        s.dev<int32_t>(oNm), window_size, nnratio, check_orientation, nullptr); }))) return rc;
    memcpy(prev_matched, s.host(oP), (size_t)n1 * 8);
    memcpy(matches12, s.host(oM), (size_t)n1 * 4);
    return *s.host<int32_t>(oNm);
}

int pgorb_search_for_initialization_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc,
                                    const int32_t* d_n, int cap, const int32_t* d_grid_start,
                                    const int32_t* d_grid_idx, const int32_t* d_pair_f1, const int32_t* d_pair_f2,
                                    int npairs, float min_x, float max_x, float min_y, float max_y,
                                    float* d_prev_matched, int32_t* d_matches12, int32_t* d_nmatches,
                                    int window_size, float nnratio, int check_orientation, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_grid_start || !d_grid_idx || npairs < 0 ||
        (npairs && (!d_pair_f1 || !d_pair_f2 || !d_prev_matched || !d_matches12 || !d_nmatches)) ||
        !(max_x > min_x) || !(max_y > min_y) || window_size < 0)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_for_initialization_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const float invW = (float)GRID_COLS / (max_x - min_x), invH = (float)GRID_ROWS / (max_y - min_y);
    const size_t ldsA = (size_t)4 * cap * 2, ldsB = (size_t)cap * 10 + 192;      // (+ the 32-bin histogram)
    if (!pg_raise_lds<k_sfi_candidates>(c, ldsA) || !pg_raise_lds<k_search_for_initialization>(c, ldsB))
        return pg_ctx_fail(c, PGORB_E_LIMIT, "SearchForInitialization state exceeds the LDS");
    PgLists Ls;                                                                    // of every F1 keypoint of every pair
    const int rc = pg_lists_acquire(c, npairs, cap, (hipStream_t)stream, &Ls);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sfi_candidates, dim3((cap + 3) / 4, npairs), dim3(256), ldsA, (hipStream_t)stream, d_kps, d_desc, d_n, cap,
                       d_grid_start, d_grid_idx, d_pair_f1, d_pair_f2, min_x, min_y, invW, invH, d_prev_matched, window_size, Ls);
    hipLaunchKernelGGL(k_search_for_initialization, dim3(npairs), dim3(64), ldsB, (hipStream_t)stream, d_kps, d_desc,
                       d_n, cap, d_grid_start, d_grid_idx, d_pair_f1, d_pair_f2, min_x, min_y, invW, invH,
                       d_prev_matched, d_matches12, d_nmatches, window_size, nnratio, check_orientation, Ls);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_search_for_initialization launch failed");
    return pg_ctx_scratch_done(c, (hipStream_t)stream);
}

int pgorb_search_by_projection_points(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x,
                                      float max_x, float min_y, float max_y, const uint8_t* kp_has_point, int npoints,
                                      const uint8_t* valid, const float* proj_x, const float* proj_y, const int32_t* level,
                                      const float* view_cos, const uint8_t* point_desc, const uint8_t* point_has_obs,
                                      float th, float nnratio, int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    return pg_search_by_projection_host(c, 0, kps, desc, n, min_x, max_x, min_y, max_y, kp_has_point, npoints, valid, proj_x, proj_y,
                                        level, view_cos, point_desc, point_has_obs, th, nnratio, 0, assigned);
}

int pgorb_search_by_projection_frame(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x,
                                     float max_x, float min_y, float max_y, const uint8_t* kp_has_point, int nlast,
                                     const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave,
                                     const float* last_angle, const uint8_t* point_desc, const uint8_t* point_has_obs,
                                     float th, int check_orientation, int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    return pg_search_by_projection_host(c, 1, kps, desc, n, min_x, max_x, min_y, max_y, kp_has_point, nlast, valid, u, v,
                                        last_octave, last_angle, point_desc, point_has_obs, th, 0.f, check_orientation, assigned);
}

int pgorb_search_by_projection_keyframe(pgorb_ctx* c, const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x,
                                        float max_x, float min_y, float max_y, const uint8_t* kp_has_point, int npoints,
                                        const uint8_t* valid, const uint8_t* already_found, const float* u, const float* v,
                                        const float* dist3d, const float* min_distance, const float* max_distance,
                                        const float* kf_angle, const uint8_t* point_desc, float log_scale_factor, float th,
                                        int orb_dist, int check_orientation, int32_t* assigned)
{
    if (!c) return PGORB_E_ARG;
    if (!(log_scale_factor > 0.0f)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_projection_keyframe: log_scale_factor must be positive");
    const PgProjKeyFrame kf = {already_found, dist3d, min_distance, max_distance, log_scale_factor, orb_dist};
    return pg_search_by_projection_host(c, 2, kps, desc, n, min_x, max_x, min_y, max_y, kp_has_point, npoints, valid, u, v, nullptr,
                                        kf_angle, point_desc, nullptr, th, 0.f, check_orientation, assigned, &kf);
}

// the contract's logarithm and the Frame's mfLogScaleFactor under it (Frame.cc:188), MapPoint::PredictScale (MapPoint.cc:516-531)
float pgorb_log_f(float x) { return pg_log_f(x); }
float pgorb_log_scale_factor(const pgorb_ctx* c)
{
    if (!c) return 0.0f;
    float sf[PG_MAXL + 1];
    pgorb_scale_tables(c, sf, nullptr, nullptr, nullptr);
    return pg_log_f(sf[1]);                              // mvScaleFactor[1] = (float)(1.0f * (double)scaleFactor) = mfScaleFactor
}
int pgorb_predict_scale(const pgorb_ctx* c, float max_distance, float current_dist)
{
    if (!c) return PGORB_E_ARG;
    return pg_predict_scale(max_distance, current_dist, pgorb_log_scale_factor(c), pgorb_levels(c));
}

int pgorb_search_by_projection_points_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point, int qcap, const int32_t* d_nq,
        const uint8_t* d_valid, const float* d_proj_x, const float* d_proj_y, const int32_t* d_level, const float* d_view_cos,
        const uint8_t* d_point_desc, const uint8_t* d_point_has_obs, float th, float nnratio, int32_t* d_assigned, int32_t* d_nmatches,
        void* stream)
{
    if (!c) return PGORB_E_ARG;
    return pg_search_by_projection_batch(c, 0, d_kps, d_desc, d_n, cap_per_frame, d_grid_start, d_grid_idx, d_pair_frame, npairs, min_x, max_x,
                                         min_y, max_y, d_kp_has_point, qcap, d_nq, d_valid, d_proj_x, d_proj_y, d_level, d_view_cos, d_point_desc,
                                         d_point_has_obs, th, nnratio, 0, d_assigned, d_nmatches, (hipStream_t)stream);
}

int pgorb_search_by_projection_frame_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point, int qcap, const int32_t* d_nq,
        const uint8_t* d_valid, const float* d_u, const float* d_v, const int32_t* d_last_octave, const float* d_last_angle,
        const uint8_t* d_point_desc, const uint8_t* d_point_has_obs, float th, int check_orientation, int32_t* d_assigned,
        int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    return pg_search_by_projection_batch(c, 1, d_kps, d_desc, d_n, cap_per_frame, d_grid_start, d_grid_idx, d_pair_frame, npairs, min_x, max_x,
                                         min_y, max_y, d_kp_has_point, qcap, d_nq, d_valid, d_u, d_v, d_last_octave, d_last_angle, d_point_desc,
                                         d_point_has_obs, th, 0.f, check_orientation, d_assigned, d_nmatches, (hipStream_t)stream);
}

int pgorb_search_by_projection_keyframe_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
        int cap_per_frame, const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point, int qcap, const int32_t* d_nq,
        const uint8_t* d_valid, const uint8_t* d_already_found, const float* d_u, const float* d_v, const float* d_dist3d,
        const float* d_min_distance, const float* d_max_distance, const float* d_kf_angle, const uint8_t* d_point_desc,
        float log_scale_factor, float th, int orb_dist, int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    const PgProjKeyFrame kf = {d_already_found, d_dist3d, d_min_distance, d_max_distance, log_scale_factor, orb_dist};
    return pg_search_by_projection_batch(c, 2, d_kps, d_desc, d_n, cap_per_frame, d_grid_start, d_grid_idx, d_pair_frame, npairs, min_x, max_x,
                                         min_y, max_y, d_kp_has_point, qcap, d_nq, d_valid, d_u, d_v, nullptr, d_kf_angle, d_point_desc,
                                         nullptr, th, 0.f, check_orientation, d_assigned, d_nmatches, (hipStream_t)stream, &kf);
}
}  // extern "C"
