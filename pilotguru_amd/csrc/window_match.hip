// window_match.hip -- the three SearchByProjection forms on gfx950, the second of the two grid-window matcher families
// (SearchForInitialization: init_match.hip; the candidate lists both build and read: cand_lists.h).
//
// Restates (thirdparty/orb-slam2):
//   Frame::GetFeaturesInArea                  src/Frame.cc:331-384
//   ORBmatcher::SearchByProjection            src/ORBmatcher.cc:46-131 (local map points), 1355-1474 (last frame), 1476-1603 (key frame)
//   ORBmatcher::ComputeThreeMaxima            src/ORBmatcher.cc:1605-1646 (match_common.h)
//   MapPoint::PredictScale                    src/MapPoint.cc:516-531
#include "proj_match.h"

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

// GetFeaturesInArea's window and the level range of query q; false = the reference skips the query
__device__ __forceinline__ bool proj_query(const PgProjBatch& B, int64_t qi, int mode, const PgGridWin& G, float& x, float& y, float& r,
                                           int& minLevel, int& maxLevel, int& cx0, int& cx1, int& cy0, int& cy1)
{
    if (!B.valid[qi]) return false;
    x = B.x[qi]; y = B.y[qi];
    int lvl;
    if (mode == 2) {
        // ORBmatcher.cc:1497-1531: not already found, projection inside the image bounds, depth inside the point's scale
        // invariance range, level from MapPoint::PredictScale
        if (B.found[qi]) return false;
        if (x < G.minX || x > B.maxX || y < G.minY || y > B.maxY) return false;          // :1512-1515
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
    return sfi_window(x, y, r, G, cx0, cx1, cy0, cy1);   // Frame.cc:336-350
}

// entry of a stored candidate: distance << 23 | rotation bin << 18 | octave << 14 | keypoint index
__device__ __forceinline__ uint32_t proj_entry(int dist, int bin, int octave, int i2)
{
    return ((uint32_t)dist << 23) | ((uint32_t)(bin & 31) << 18) | ((uint32_t)(octave & 15) << 14) | (uint32_t)i2;
}
static_assert(LIST_MAX_N <= (1 << 14), "the index field of an entry");
__device__ __forceinline__ int proj_index(uint32_t e) { return (int)(e & 0x3FFFu); }
__device__ __forceinline__ int proj_dist(uint32_t e) { return (int)(e >> 23); }
__device__ __forceinline__ int proj_octave(uint32_t e) { return (int)((e >> 14) & 15u); }
__device__ __forceinline__ int proj_bin(uint32_t e) { return (int)((e >> 18) & 31u); }

// Pass A: workgroup = 4 waves = 4 consecutive queries of pair blockIdx.y
__global__ __launch_bounds__(256) void k_proj_candidates(PgProjBatch B, PgGridWin G, int mode, PgLists Ls)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, p = blockIdx.y;
    const int q = blockIdx.x * 4 + wv;
    const int nq = min(B.nq[p], B.qcap);
    if (q >= nq) return;
    const int frame = B.pairFrame ? B.pairFrame[p] : p, cap = B.cap;
    const int64_t qi = (int64_t)p * B.qcap + q;
    float x, y, r; int minLevel, maxLevel, cx0, cx1, cy0, cy1;
    if (!proj_query(B, qi, mode, G, x, y, r, minLevel, maxLevel, cx0, cx1, cy0, cy1)) {
        if (lane == 0) Ls.cnt[qi] = 0;
        return;
    }
    const pgorb_keypoint* __restrict__ K = B.K + (int64_t)frame * cap;
    const uint8_t* __restrict__ D = B.D + (int64_t)frame * cap * 32;
    uint16_t* candList = reinterpret_cast<uint16_t*>(pg_sfi_smem) + (size_t)wv * cap;
    const int M = pg_window_gather(B.gstart + (int64_t)frame * (GRID_CELLS + 1), B.gidx + (int64_t)frame * cap, cx0, cx1, cy0, cy1, candList, lane);
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const uint4 q0 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[1];
    const float qangle = mode != 0 ? B.aux[qi] : 0.f;
    pg_list_build(Ls, qi, p, M, lane, [&](int k, uint32_t& e) {
        const int i2 = candList[k];
        const pgorb_keypoint kp2 = K[i2];
        const bool ok = !(bCheckLevels && (kp2.octave < minLevel || (maxLevel >= 0 && kp2.octave > maxLevel))) &&
                        fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r;
        e = ok ? proj_entry(sfi_distance(q0, q1, D + (int64_t)i2 * 32), mode != 0 ? pg_rot_bin(qangle, kp2.angle) : 0, kp2.octave, i2) : 0u;
        return ok;
    });
}

// a query whose list did not fit its pair's pool: the whole evaluation in place, in the reference's order (the round-2 form of the
// kernel); returns the best two entries, their keys' distances in the entry's distance field
__device__ __noinline__ uint2 proj_eval_in_place(const PgProjBatch B, int64_t qi, int frame, int mode, const PgGridWin G, const uint8_t* taken, int lane)
{
    float x, y, r; int minLevel, maxLevel, cx0, cx1, cy0, cy1;
    proj_query(B, qi, mode, G, x, y, r, minLevel, maxLevel, cx0, cx1, cy0, cy1);      // (true: pass A got here)
    const int cap = B.cap;
    const pgorb_keypoint* K = B.K + (int64_t)frame * cap;
    const uint8_t* D = B.D + (int64_t)frame * cap * 32;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const uint4 q0 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[0];
    const uint4 q1 = reinterpret_cast<const uint4*>(B.desc + qi * 32)[1];
    const float qangle = mode != 0 ? B.aux[qi] : 0.f;
    unsigned long long b1 = ~0ull, b2 = ~0ull;              // (distance << 48 | scan position << 32 | entry): the lane's two smallest
    pg_window_walk(B.gstart + (int64_t)frame * (GRID_CELLS + 1), B.gidx + (int64_t)frame * cap, cx0, cx1, cy0, cy1, lane, [&](int i2, int pos) {
        const pgorb_keypoint kp2 = K[i2];
        if (bCheckLevels && (kp2.octave < minLevel || (maxLevel >= 0 && kp2.octave > maxLevel))) return;
        if (!(fabsf(__fsub_rn(kp2.x, x)) < r && fabsf(__fsub_rn(kp2.y, y)) < r)) return;
        if (taken[i2]) return;
        const int dist = sfi_distance(q0, q1, D + (int64_t)i2 * 32);
        const unsigned long long key = ((unsigned long long)dist << 48) | ((unsigned long long)pos << 32) |
                                       proj_entry(dist, mode != 0 ? pg_rot_bin(qangle, kp2.angle) : 0, kp2.octave, i2);
        b2 = key < b1 ? b1 : (key < b2 ? key : b2);
        b1 = key < b1 ? key : b1;
    });
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
    PgProjBatch B, PgGridWin G, int mode, float nnratio, int checkOrientation, PgLists Ls, int32_t* __restrict__ assignedOut, int32_t* __restrict__ nmatchesOut)
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
        // four of the undecided queries at a time per wave, their lists in flight together: the query (-1: none left), its list's
        // length and entry `lane` of its fixed slots
        auto four_queries = [&](int u0, int (&q)[4], int (&c)[4], uint32_t (&e)[4]) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                q[j] = u0 + j < nun ? (int)cur[u0 + j] : -1;
                c[j] = q[j] >= 0 ? (int)cntL[q[j]] : 0;
                e[j] = (c[j] != (int)LIST_OVER && lane < min(c[j], LIST_K)) ? Ls.fixed[(qo + q[j]) * LIST_K + lane] : 0u;
            }
        };
        // ---- takeable candidates of every undecided query ----
        for (int u0 = wv * 4; u0 < nun; u0 += RR_W * 4) {
            int q[4], c[4]; uint32_t e[4];
            four_queries(u0, q, c, e);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (q[j] < 0) break;
                if (lane == 0) atomicMin(&ctrl[4], q[j]);
                if (c[j] == (int)LIST_OVER) { if (lane == 0) atomicMin(&ctrl[3], q[j]); continue; }
                const uint32_t ovf = c[j] > LIST_K ? Ls.ovf[qo + q[j]] : 0u;
                pg_list_chunks(c[j], e[j], pg_list_tail(Ls, p, ovf), lane, [&](int, uint32_t ee, bool inRange) {
                    if (inRange) {
                        if (mode == 0) atomicMin(&minAny[proj_index(ee)], (uint32_t)q[j]);
                        if (proj_dist(ee) <= thTake) atomicMin(&minq[proj_index(ee)], (uint32_t)q[j]);
                    }
                    return true;
                });
            }
        }
        __syncthreads();
        const int minOver = ctrl[3], minAll = ctrl[4];
        // ---- ready queries decide ----
        for (int u0 = wv * 4; u0 < nun; u0 += RR_W * 4) {
            int q[4], c[4]; uint32_t e[4];
            four_queries(u0, q, c, e);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int qq = q[j];
                if (qq < 0) break;
                const bool isOver = c[j] == (int)LIST_OVER;
                const uint32_t ovf = (!isOver && c[j] > LIST_K) ? Ls.ovf[qo + qq] : 0u;
                bool ready = isOver ? (qq == minAll) : (qq < minOver);
                if (ready && !isOver)
                    pg_list_chunks(c[j], e[j], pg_list_tail(Ls, p, ovf), lane, [&](int, uint32_t ee, bool inRange) {
                        // (mode 0 only: a query must not take a keypoint an undecided EARLIER query still has to read -- the second best of
                        //  its ratio test looks at candidates beyond TH_HIGH too; the best-only forms decide the same either way)
                        const bool blocked = minq[proj_index(ee)] < (uint32_t)qq ||
                                             (mode == 0 && proj_dist(ee) <= thTake && minAny[proj_index(ee)] < (uint32_t)qq);
                        if (__ballot(inRange && blocked) != 0ull) ready = false;
                        return ready;
                    });
                if (!ready) { if (lane == 0) nxt[atomicAdd(&ctrl[1 - curC], 1)] = (uint16_t)qq; continue; }
                // best and second best of the candidates that hold no point (:79-81 / :1397-1399 / :1542-1543); first minimum wins:
                // key = distance << 16 | position in the list
                uint32_t e1 = 0xFFFFFFFFu, e2 = 0xFFFFFFFFu;
                if (!isOver) {
                    unsigned w1 = 0xFFFFFFFFu, w2 = 0xFFFFFFFFu;
                    pg_list_chunks(c[j], e[j], pg_list_tail(Ls, p, ovf), lane, [&](int ch, uint32_t ee, bool inRange) {
                        const bool keep = inRange && !taken[proj_index(ee)];
                        const unsigned key = keep ? (((unsigned)proj_dist(ee) << 16) | (unsigned)(ch * 64 + lane)) : 0xFFFFFFFFu;
                        unsigned k1, k2;
                        wave_min2_u32(key, k1, k2);
                        const uint32_t c1 = k1 == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readlane((int)ee, (int)(k1 & 63u));
                        const uint32_t c2 = k2 == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readlane((int)ee, (int)(k2 & 63u));
                        // (merged on copies and stored back once: branches that store k1 to w1 here and to w2 there keep all four in scratch memory)
                        unsigned n1 = w1, n2 = w2; uint32_t f1 = e1, f2 = e2;
                        if (k1 < n1) {
                            if (n1 < k2) { n2 = n1; f2 = f1; } else { n2 = k2; f2 = c2; }
                            n1 = k1; f1 = c1;
                        } else if (k1 < n2) { n2 = k1; f2 = c1; }
                        w1 = n1; w2 = n2; e1 = f1; e2 = f2;
                        return true;
                    });
                } else {
                    const uint2 ev = proj_eval_in_place(B, qo + qq, frame, mode, G, taken, lane);
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

int pg_proj_begin(pgorb_ctx* c, int cap, int qcap, int npairs, size_t extraBytes, hipStream_t stream, PgLists* Ls, void** extra)
{
    assert(cap <= LIST_MAX_N);                               // (the entries' 14-bit index; qcap: pg_lists_acquire)
    return pg_lists_acquire<k_proj_candidates, k_search_by_projection>(c, npairs, std::max(qcap, 1), (size_t)4 * cap * 2, pg_sbp_lds(cap, qcap),
                                                                       PG_SBP_LDS_MSG, extraBytes, stream, Ls, extra);
}

int pg_proj_run(pgorb_ctx* c, PgProjBatch& B, int npairs, float min_x, float max_x, float min_y, float max_y, int mode, float nnratio,
                int check_orientation, const PgLists& Ls, int32_t* d_assigned, int32_t* d_nmatches, hipStream_t stream)
{
    B.nlevels = pgorb_levels(c); B.maxX = max_x; B.maxY = max_y;
    pgorb_scale_tables(c, B.sf, nullptr, nullptr, nullptr);
    const PgGridWin G = pg_grid_win(min_x, max_x, min_y, max_y);
    const int cap = B.cap, qcap = B.qcap;
    if (qcap) hipLaunchKernelGGL(k_proj_candidates, dim3((qcap + 3) / 4, npairs), dim3(256), (size_t)4 * cap * 2, stream, B, G, mode, Ls);
    hipLaunchKernelGGL(k_search_by_projection, dim3(npairs), dim3(RR_T), pg_sbp_lds(cap, qcap), stream, B, G, mode, nnratio, check_orientation, Ls,
                       d_assigned, d_nmatches);
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
    if (cap > LIST_MAX_N || qcap > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
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
    if (n > LIST_MAX_N || nq > LIST_MAX_N) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints / queries");
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
