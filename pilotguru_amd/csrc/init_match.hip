// init_match.hip -- SearchForInitialization on gfx950, the first of the two grid-window matcher families (the SearchByProjection forms:
// window_match.hip; the candidate lists both build and read: cand_lists.h).
//
// Restates (thirdparty/orb-slam2):
//   Frame::GetFeaturesInArea                  src/Frame.cc:331-384
//   ORBmatcher::SearchForInitialization       src/ORBmatcher.cc:407-522
//   ORBmatcher::ComputeThreeMaxima            src/ORBmatcher.cc:1605-1646 (match_common.h)
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
#include "cand_lists.h"

// Batch layout of the two passes: pair p matches frame pairF1[p] against frame pairF2[p] of an extract batch (keypoints / descriptors
// `cap` apart, grids (GRID_CELLS + 1) / cap apart); prevMatched is [npairs][cap][2], the lists have `cap` rows a pair.
struct PgSfiBatch {
    const pgorb_keypoint* kps; const uint8_t* desc; const int32_t* nper; int cap;
    const int32_t* gstart; const int32_t* gidx; const int32_t* pairF1; const int32_t* pairF2;
    PgGridWin G; float* prevMatched; int windowSize;
};
// frame f of the batch as a pair reads it.  (The out-of-line evaluators take this and the grid, not the batch: an argument block of
// more than 16 registers reaches a non-inlined function through scratch memory, like the reference parameters of the note below.)
struct PgSfiFrame { const pgorb_keypoint* K; const uint8_t* D; const int32_t* start; const int32_t* idx; };
__device__ __forceinline__ PgSfiFrame sfi_frame(const PgSfiBatch& B, int f)
{
    return PgSfiFrame{B.kps + (int64_t)f * B.cap, B.desc + (int64_t)f * B.cap * 32, B.gstart + (int64_t)f * (GRID_CELLS + 1),
                      B.gidx + (int64_t)f * B.cap};
}

// entry of a stored candidate: distance << 16 | keypoint index
static_assert(LIST_MAX_N <= (1 << 16), "the index field of an entry");
__device__ __forceinline__ uint32_t sfi_entry(int dist, int i2) { return ((uint32_t)dist << 16) | (uint32_t)i2; }
__device__ __forceinline__ int sfi_entry_index(uint32_t e) { return (int)(e & 0xFFFFu); }
__device__ __forceinline__ int sfi_entry_dist(uint32_t e) { return (int)(e >> 16); }

// Phase 1: candidate lists.  Workgroup = 4 waves = 4 consecutive F1 keypoints of pair blockIdx.y.
__global__ __launch_bounds__(256) void k_sfi_candidates(PgSfiBatch B, PgLists Ls)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, p = blockIdx.y, cap = B.cap;
    const int i1 = blockIdx.x * 4 + wv;
    const int f1 = B.pairF1[p], f2 = B.pairF2[p];
    const int n1 = min(B.nper[f1], cap);
    if (i1 >= n1) return;
    const int64_t row = (int64_t)p * cap + i1;
    const int level1 = B.kps[(int64_t)f1 * cap + i1].octave;
    int cx0, cx1, cy0, cy1;
    const float x = B.prevMatched[row * 2], y = B.prevMatched[row * 2 + 1];
    const float r = (float)B.windowSize;
    if (level1 > 0 || !sfi_window(x, y, r, B.G, cx0, cx1, cy0, cy1)) {        // :424-426
        if (lane == 0) Ls.cnt[row] = 0;
        return;
    }
    const PgSfiFrame F2 = sfi_frame(B, f2);
    uint16_t* candList = reinterpret_cast<uint16_t*>(pg_sfi_smem) + (size_t)wv * cap;      // this wave's vIndices2 before filtering
    const int M = pg_window_gather(F2.start, F2.idx, cx0, cx1, cy0, cy1, candList, lane);
    const uint4 q0 = reinterpret_cast<const uint4*>(B.desc + ((int64_t)f1 * cap + i1) * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.desc + ((int64_t)f1 * cap + i1) * 32)[1];
    // bCheckLevels is true for minLevel = maxLevel = 0 (Frame.cc:354): octave must equal level1
    pg_list_build(Ls, row, p, M, lane, [&](int k, uint32_t& e) {
        const int i2 = candList[k];
        const pgorb_keypoint kp2 = F2.K[i2];
        const bool ok = kp2.octave == level1 && fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r;
        e = ok ? sfi_entry(sfi_distance(q0, q1, F2.D + (int64_t)i2 * 32), i2) : 0u;
        return ok;
    });
}

// A keypoint of F1 with more than LIST_K candidates in its window (rare: every keypoint of a dense patch within 100 px):
// distances and the vMatchedDistance filter evaluated in place, cell by cell in the reference's (column, row, insertion)
// order.  Out: smallest (distance << 16 | running position), the second-smallest distance, the winner's i2.
// (results by value: reference parameters of a non-inlined function live in scratch memory, and the common path paid for it)
__device__ __noinline__ uint3 sfi_eval_in_place(const PgGridWin G, const PgSfiFrame F2, int level1, float x, float y, float r, const uint8_t* d1,
                                                const uint16_t* matchedDist, int lane)
{
    int cx0, cx1, cy0, cy1;
    sfi_window(x, y, r, G, cx0, cx1, cy0, cy1);          // (true: phase 1 got here)
    const uint4 q0 = reinterpret_cast<const uint4*>(d1)[0], q1 = reinterpret_cast<const uint4*>(d1)[1];
    unsigned b1key = 0xFFFFFFFFu, b1idx = 0; int b2 = 0x7fffffff;
    pg_window_walk(F2.start, F2.idx, cx0, cx1, cy0, cy1, lane, [&](int i2, int pos) {
        const pgorb_keypoint kp2 = F2.K[i2];
        const float distx = __fsub_rn(kp2.x, x), disty = __fsub_rn(kp2.y, y);
        if (kp2.octave != level1 || !(fabsf(distx) < r && fabsf(disty) < r)) return;
        const int dist = sfi_distance(q0, q1, F2.D + (int64_t)i2 * 32);
        if ((int)matchedDist[i2] <= dist) return;
        const unsigned key = ((unsigned)dist << 16) | (unsigned)pos;     // pos < cap < 2^16
        if (key < b1key) { if (b1key != 0xFFFFFFFFu) b2 = min(b2, (int)(b1key >> 16)); b1key = key; b1idx = (unsigned)i2; }
        else b2 = min(b2, dist);
    });
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
__device__ __noinline__ uint3 sfi_eval_long(int count, uint32_t e0, const uint32_t* tail, const PgGridWin G, const PgSfiFrame F2, int level1,
                                            float x, float y, float r, const uint8_t* d1, const uint16_t* matchedDist, int lane)
{
    if (count == (int)LIST_OVER) return sfi_eval_in_place(G, F2, level1, x, y, r, d1, matchedDist, lane);
    unsigned wkey = 0xFFFFFFFFu, second = 0xFFFFFFFFu;
    int bestIdx2 = -1;
    pg_list_chunks(count, e0, tail, lane, [&](int ch, uint32_t ee, bool inRange) {
        const int i2 = sfi_entry_index(ee), dist = sfi_entry_dist(ee);
        const bool keep = inRange && !((int)matchedDist[i2] <= dist);       // :445-446
        const unsigned key = keep ? (((unsigned)dist << 16) | (unsigned)(ch * 64 + lane)) : 0xFFFFFFFFu;
        unsigned k1, k2;
        wave_min2_u32(key, k1, k2);
        if (k1 < wkey) { second = min(wkey, k2); wkey = k1; bestIdx2 = __builtin_amdgcn_readlane(i2, (int)(k1 & 63u)); }
        else second = min(second, k1);
        return true;
    });
    return make_uint3(wkey, second == 0xFFFFFFFFu ? 0x7fffffffu : (second >> 16), (unsigned)bestIdx2);
}

#define SFI_G 8                  // keypoints per prefetch group
// Phase 2: the sequential pass, one wave per pair.  (Round 4 also built this pass as ROUNDS of independent keypoints -- the scheme
// k_search_by_projection runs (window_match.hip) -- and measured it slower here: every listed keypoint of a pair is a level-0 keypoint with a
// 200-px window, the lists overlap heavily, and the conservative readiness rule left ~10 % of the keypoints per round: 1.33 ms per 127
// pairs of 4 000 features against 0.68 ms for this walk; profiles/r04_next_tier.txt.  The lists are variable length now: a dense
// window no longer falls back to the evaluation in place.)
__global__ __launch_bounds__(64) void k_search_for_initialization(
    PgSfiBatch B, int32_t* __restrict__ matches12out, int32_t* __restrict__ nmatchesOut, float nnratio, int checkOrientation, PgLists Ls)
{
    const int lane = threadIdx.x, p = blockIdx.x, cap = B.cap;
    const int f1 = B.pairF1[p], f2 = B.pairF2[p];
    const int n1 = min(B.nper[f1], cap);
    const PgSfiFrame F1 = sfi_frame(B, f1), F2 = sfi_frame(B, f2);
    float* prev = B.prevMatched + (int64_t)p * cap * 2;
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

    const float r = (float)B.windowSize;
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
                E[j] = L[(int64_t)i1 * LIST_K + lane];                        // (all 64 slots: no wait for the count; slots past it are masked below)
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
                const int i2 = sfi_entry_index(curE[j]), dist = sfi_entry_dist(curE[j]);
                const bool keep = lane < curC[j] && !((int)matchedDist[i2] <= dist);       // :445-446
                const unsigned key = keep ? (((unsigned)dist << 16) | (unsigned)lane) : 0xFFFFFFFFu;
                wave_min2_u32(key, wkey, second);                           // smallest key, and the smallest of the others
                if (wkey == 0xFFFFFFFFu) continue;
                bestIdx2 = __builtin_amdgcn_readlane(i2, (int)(wkey & 0xFFFFu));
                second = (second == 0xFFFFFFFFu) ? 0x7fffffffu : (second >> 16);
            } else {
                // a dense window (the list continues in the pair's pool) or a pair whose pool is full (evaluation in place): out of line, so
                // that the eight unrolled copies of this body stay small -- inlined, the sequential wave lost 20 % to instruction fetch
                const uint3 ev = sfi_eval_long(curC[j], curE[j], pg_list_tail(Ls, p, Ls.ovf[row0 + i1]), B.G, F2, F1.K[i1].octave, prev[2 * i1],
                                               prev[2 * i1 + 1], r, F1.D + (int64_t)i1 * 32, matchedDist, lane);
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
                if (i2v[u] >= 0) { a1[u] = F1.K[i].angle; a2[u] = F2.K[i2v[u]].angle; }
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
            if (mv[u] >= 0) xy[u] = *reinterpret_cast<const float2*>(&F2.K[mv[u]].x);
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
    if (cap > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");      // (before anything is staged)
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
    if (cap > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    const size_t ldsA = (size_t)4 * cap * 2, ldsB = (size_t)cap * 10 + 192;      // (+ the 32-bin histogram)
    PgLists Ls;                                                                    // of every F1 keypoint of every pair
    const int rc = pg_lists_acquire<k_sfi_candidates, k_search_for_initialization>(c, npairs, cap, ldsA, ldsB, "SearchForInitialization state exceeds the LDS",
                                                                                   0, (hipStream_t)stream, &Ls, nullptr);
    if (rc) return rc;
    const PgSfiBatch B = {d_kps, d_desc, d_n, cap, d_grid_start, d_grid_idx, d_pair_f1, d_pair_f2, pg_grid_win(min_x, max_x, min_y, max_y),
                          d_prev_matched, window_size};
    hipLaunchKernelGGL(k_sfi_candidates, dim3((cap + 3) / 4, npairs), dim3(256), ldsA, (hipStream_t)stream, B, Ls);
    hipLaunchKernelGGL(k_search_for_initialization, dim3(npairs), dim3(64), ldsB, (hipStream_t)stream, B, d_matches12, d_nmatches, nnratio,
                       check_orientation, Ls);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_search_for_initialization launch failed");
    return pg_ctx_scratch_done(c, (hipStream_t)stream);
}
}  // extern "C"
