// node_match.hip -- the BoW-node matchers on gfx950: the FeatureVector of a frame, both SearchByBoW forms and SearchForTriangulation.
//
// Restates (thirdparty/orb-slam2):
//   DBoW2 FeatureVector::addFeature           Thirdparty/DBoW2/DBoW2/FeatureVector.cpp:31-45
//   ORBmatcher::SearchByBoW(KeyFrame*, Frame&) src/ORBmatcher.cc:161-290
//   ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*) src/ORBmatcher.cc:524-657
//   ORBmatcher::SearchForTriangulation        src/ORBmatcher.cc:659-825, 142-159
//   ORBmatcher::ComputeThreeMaxima            src/ORBmatcher.cc:1605-1646 (match_common.h)
// All three walk the vocabulary nodes two frames share, one wave per node, and end in k_match_finish.  mapping.hip reaches
// SearchForTriangulation through pg_tri_launch.
#include "match_common.h"

// FeatureVector of every frame of a batch (DBoW2 FeatureVector::addFeature, FeatureVector.cpp:31-45, as
// TemplatedVocabulary::transform fills it, TemplatedVocabulary.h:1180-1186): map<node id, vector<feature index>> with the
// indices appended in feature order = the features sorted by (node id, index), as CSR.  One workgroup per frame: rank of
// every feature by counting (n <= a few thousand: n^2 / 1024 compares per thread on LDS), scatter, group heads by a scan.
__global__ __launch_bounds__(1024) void k_feature_vectors(const uint32_t* __restrict__ node, const int32_t* __restrict__ nIn, int cap,
                                                          uint32_t* __restrict__ fvNode, int32_t* __restrict__ fvStart,
                                                          uint32_t* __restrict__ fvFeat, int32_t* __restrict__ nfv)
{
    const int f = blockIdx.x, tid = threadIdx.x, n = min(nIn[f], cap);
    uint32_t* key = reinterpret_cast<uint32_t*>(pg_sfi_smem);            // [cap] node id of feature i
    uint32_t* snode = key + cap;                                          // [cap] sorted node ids
    int* scan = reinterpret_cast<int*>(snode + cap);                      // [1024 + 1]
    node += (int64_t)f * cap; fvNode += (int64_t)f * cap; fvFeat += (int64_t)f * cap; fvStart += (int64_t)f * (cap + 1);
    for (int i = tid; i < n; i += 1024) key[i] = node[i];
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const uint32_t k = key[i];
        int r = 0;
        for (int j = 0; j < n; j++) { const uint32_t kj = key[j]; r += (kj < k) || (kj == k && j < i); }
        snode[r] = k; fvFeat[r] = (uint32_t)i;
    }
    __syncthreads();
    // group heads: position r starts a group when its node differs from its predecessor's; exclusive scan of the flags
    const int per = (n + 1023) / 1024, r0 = tid * per, r1 = min(n, r0 + per);
    int heads = 0;
    for (int r = r0; r < r1; r++) heads += (r == 0 || snode[r] != snode[r - 1]);
    scan[tid] = heads;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int t = 0; t < 1024; t++) { const int h = scan[t]; scan[t] = acc; acc += h; } scan[1024] = acc; }
    __syncthreads();
    int g = scan[tid];
    for (int r = r0; r < r1; r++)
        if (r == 0 || snode[r] != snode[r - 1]) { fvNode[g] = snode[r]; fvStart[g] = r; g++; }
    if (tid == 0) { fvStart[scan[1024]] = n; nfv[f] = scan[1024]; }
}

// The same CSR by SORTING (round 4; round 5: the sort is this file's own): the features' keys node id << 13 | feature index are
// unique, the features arrive in index order, so the FeatureVector is a STABLE sort by node id.  One workgroup per frame holds up to
// FV_T * FV_IPT = 8 192 keys in LDS and runs least-significant-digit passes of 2 bits over exactly the bits the largest node id uses
// (ORBvoc at levelsup 4: 11 bits, six passes): a thread owns 8 CONSECUTIVE positions (stability), counts its four digits in two
// packed 16 + 16-bit words (a count never exceeds 8 192), one DPP wave scan per word + sixteen wave totals give every thread the
// number of equal digits in front of it, and the keys are scattered into the second buffer.  (Round 4 called rocPRIM's
// block_radix_sort here; the counting form above is O(n^2) -- 0.17 ms for 128 frames of 2 000 features, 0.65 ms at 4 000 -- and stays
// for frames beyond 8 192 features.)
#define FV_T 1024
#define FV_IPT 8
__global__ __launch_bounds__(FV_T) void k_feature_vectors_sorted(const uint32_t* __restrict__ node, const int32_t* __restrict__ nIn, int cap,
                                                                 uint32_t* __restrict__ fvNode, int32_t* __restrict__ fvStart,
                                                                 uint32_t* __restrict__ fvFeat, int32_t* __restrict__ nfv)
{
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = min(nIn[f], cap);
    unsigned long long* bufA = reinterpret_cast<unsigned long long*>(pg_sfi_smem);                      // [FV_T * FV_IPT] keys
    unsigned long long* bufB = bufA + FV_T * FV_IPT;
    uint32_t* snode = reinterpret_cast<uint32_t*>(bufB);                                                  // the sorted node ids end up here
    int* wsum = reinterpret_cast<int*>(bufB + FV_T * FV_IPT);                                             // [2 * FV_T / 64 + 2]
    node += (int64_t)f * cap; fvNode += (int64_t)f * cap; fvFeat += (int64_t)f * cap; fvStart += (int64_t)f * (cap + 1);
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < FV_IPT; k++) {
        const int i = tid * FV_IPT + k;
        const uint32_t nd = i < n ? node[i] : 0u;
        mx = max(mx, nd);
        bufA[i] = i < n ? (((unsigned long long)nd << 13) | (unsigned long long)i) : 0xFFFFFFFFFFFFFFFFull;      // padding: all ones, stays last
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    if (lane == 0) wsum[wv] = (int)mx;
    __syncthreads();
    for (int w = 0; w < FV_T / 64; w++) mx = max(mx, (uint32_t)wsum[w]);
    __syncthreads();
    const int nbits = 32 - __clz(mx | 1u);                      // bits of the largest node id
    unsigned long long *src = bufA, *dst = bufB;
    for (int shift = 13; shift < 13 + nbits; shift += 2) {
        unsigned long long key[FV_IPT];
        uint32_t c01 = 0u, c23 = 0u, before[FV_IPT];            // packed digit counts of this thread: (digit 0 | digit 1 << 16), (2 | 3 << 16)
#pragma unroll
        for (int k = 0; k < FV_IPT; k++) {
            key[k] = src[tid * FV_IPT + k];
            const uint32_t d = (uint32_t)(key[k] >> shift) & 3u, fld = (d & 1u) << 4;
            const uint32_t word = (d & 2u) ? c23 : c01;
            before[k] = (word >> fld) & 0xFFFFu;                // equal digits of this thread in front of key k
            if (d & 2u) c23 += 1u << fld; else c01 += 1u << fld;
        }
        const uint32_t i01 = (uint32_t)wave_incl_scan((int)c01, lane), i23 = (uint32_t)wave_incl_scan((int)c23, lane);
        if (lane == 63) { wsum[2 * wv] = (int)i01; wsum[2 * wv + 1] = (int)i23; }
        __syncthreads();
        uint32_t b01 = 0u, b23 = 0u, t01 = 0u, t23 = 0u;        // digits in the waves in front of this one / in the whole block
        for (int w = 0; w < FV_T / 64; w++) {
            const uint32_t v01 = (uint32_t)wsum[2 * w], v23 = (uint32_t)wsum[2 * w + 1];
            if (w < wv) { b01 += v01; b23 += v23; }
            t01 += v01; t23 += v23;
        }
        const uint32_t e01 = b01 + i01 - c01, e23 = b23 + i23 - c23;             // exclusive over the threads, still packed
        const uint32_t base1 = t01 & 0xFFFFu, base2 = base1 + (t01 >> 16), base3 = base2 + (t23 & 0xFFFFu);
#pragma unroll
        for (int k = 0; k < FV_IPT; k++) {
            const uint32_t d = (uint32_t)(key[k] >> shift) & 3u, fld = (d & 1u) << 4;
            const uint32_t ex = (((d & 2u) ? e23 : e01) >> fld) & 0xFFFFu;
            const uint32_t base = d == 0u ? 0u : d == 1u ? base1 : d == 2u ? base2 : base3;
            dst[base + ex + before[k]] = key[k];
        }
        __syncthreads();
        unsigned long long* t = src; src = dst; dst = t;
    }
    unsigned long long skey[FV_IPT];
#pragma unroll
    for (int k = 0; k < FV_IPT; k++) skey[k] = src[tid * FV_IPT + k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FV_IPT; k++) {
        const int r = tid * FV_IPT + k;
        if (r < n) { snode[r] = (uint32_t)(skey[k] >> 13); fvFeat[r] = (uint32_t)(skey[k] & 8191ull); }
    }
    __syncthreads();
    // group heads: position r starts a group when its node differs from its predecessor's; exclusive scan of the counts over the threads
    int heads = 0;
#pragma unroll
    for (int k = 0; k < FV_IPT; k++) { const int r = tid * FV_IPT + k; heads += (r < n && (r == 0 || snode[r] != snode[r - 1])) ? 1 : 0; }
    const int incl = wave_incl_scan(heads, lane);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < FV_T / 64; w++) { const int v = wsum[w]; base += w < wv ? v : 0; total += v; }
    int g = base + incl - heads;
#pragma unroll
    for (int k = 0; k < FV_IPT; k++) {
        const int r = tid * FV_IPT + k;
        if (r < n && (r == 0 || snode[r] != snode[r - 1])) { fvNode[g] = snode[r]; fvStart[g] = r; g++; }
    }
    if (tid == 0) { fvStart[total] = n; nfv[f] = total; }
}

// ---- SearchByBoW(KeyFrame*, Frame&), src/ORBmatcher.cc:161-290 -----------------------------------
// One wave per (key frame, frame) pair: merge-join of the two node lists; inside a common node the
// key frame's features are visited in order (each assignment removes a candidate for the later
// ones, :211-212) and the frame's features of that node are scanned one per lane.
// Batch layout (round 3): pair p = blockIdx.x, key frame pairKF[p] and frame pairF[p] of ONE extract batch (descriptors and
// keypoint angles `cap` apart); the FeatureVectors are the per-frame CSR arrays k_feature_vectors builds on the device
// (fvNode / fvFeat `cap` apart, fvStart cap + 1 apart); kfValid and the outputs are [npairs][cap].
struct PgBowBatch {
    PgFvBatch fv;
    const int32_t* pairKF; const int32_t* pairF; const uint8_t* kfValid;
};

// Round 3: NODES in parallel.  A frame feature belongs to exactly one vocabulary node, so the reference's order dependence
// ("vpMapPointMatches[realIdxF] already set", :219-220) never crosses a node: one wave walks ONE common node -- its key-frame
// features in order, the frame's features of the node one per lane and held in registers (descriptor, angle, "already
// matched" bit) for the whole walk -- and all nodes of all pairs run side by side.  A finishing wave per pair counts the
// matches and applies the rotation histogram (:256-277).  (The one-wave-per-pair form walked all ~2000 key-frame features of a
// pair in a row with the descriptor reads inside the chain: 1.34 ms per 127 pairs; a two-pass form like SearchByProjection's
// did not help because most features sit in nodes with more than 64 frame features.)
#define BOW_R 4                  // frame features per lane held in registers: nodes of up to 256 frame features
#define BOW_WAVES 64             // waves per pair, each takes the nodes a = wave, wave + 64, ...

// a frame of the batch as the node walk sees it: its FeatureVector (node ids, the nodes' starts, the features) and its keypoints and descriptors
struct PgFvView { const uint32_t* node; const int32_t* start; const uint32_t* feat; int nfv; const pgorb_keypoint* K; const uint8_t* D; };
__device__ __forceinline__ PgFvView pg_fv_view(const PgFvBatch& B, int f)
{
    const int64_t o = (int64_t)f * B.cap;
    return {B.fvNode + o, B.fvStart + (int64_t)f * (B.cap + 1), B.fvFeat + o, B.nfv[f], B.K + o, B.D + o * 32};
}
// the entry of node `id` in a frame's node list (it ascends), or -1
__device__ __forceinline__ int pg_fv_find_node(const PgFvView& v, uint32_t id)
{
    int lo = 0, hi = v.nfv;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (v.node[mid] < id) lo = mid + 1; else hi = mid; }
    return (lo < v.nfv && v.node[lo] == id) ? lo : -1;
}

__global__ __launch_bounds__(64) void k_search_by_bow(PgBowBatch B, float nnratio, int checkOrientation,
                                                       int32_t* __restrict__ matchesOut, int8_t* __restrict__ binOut)
{
    const int p = blockIdx.y, cap = B.fv.cap;
    const PgFvView kf = pg_fv_view(B.fv, B.pairKF[p]), fr = pg_fv_view(B.fv, B.pairF[p]);
    const uint8_t* __restrict__ kfValid = B.kfValid + (int64_t)p * cap;
    matchesOut += (int64_t)p * cap; binOut += (int64_t)p * cap;
    const int lane = threadIdx.x;
    for (int a = blockIdx.x; a < kf.nfv; a += BOW_WAVES) {
        const int lo = pg_fv_find_node(fr, kf.node[a]);                  // the frame's entry of the same node
        if (lo < 0) continue;
        const int a0 = kf.start[a], a1 = kf.start[a + 1], b0 = fr.start[lo], b1 = fr.start[lo + 1], nb = b1 - b0;
        const bool inRegs = nb <= 64 * BOW_R;
        // the frame's features of the node: lane holds candidates k = lane, lane + 64, ... (k = position in the node's list)
        uint4 d0[BOW_R], d1[BOW_R]; float ang[BOW_R]; int idxF[BOW_R];
        unsigned takenBits = 0;
#pragma unroll
        for (int r = 0; r < BOW_R; r++) {
            const int k = 64 * r + lane;
            idxF[r] = -1; ang[r] = 0.f; d0[r] = make_uint4(0, 0, 0, 0); d1[r] = d0[r];
            if (inRegs && k < nb) {
                idxF[r] = (int)fr.feat[b0 + k];
                d0[r] = reinterpret_cast<const uint4*>(fr.D + (int64_t)idxF[r] * 32)[0];
                d1[r] = reinterpret_cast<const uint4*>(fr.D + (int64_t)idxF[r] * 32)[1];
                ang[r] = fr.K[idxF[r]].angle;
            }
        }
        // The key frame's features of the node, one after the other.  Each needs its index (kf.feat), then its descriptor and validity
        // through that index: two dependent global round trips, ~2 us per feature when they sat inside the iteration -- most of this
        // kernel's time.  They run two iterations / one iteration ahead instead (all lanes load the same addresses).
        int idxN = a0 < a1 ? (int)kf.feat[a0] : 0, idxN2 = a0 + 1 < a1 ? (int)kf.feat[a0 + 1] : 0;
        uint4 nq0 = make_uint4(0, 0, 0, 0), nq1 = nq0;
        uint8_t nvalid = 0;
        if (a0 < a1) {
            nq0 = reinterpret_cast<const uint4*>(kf.D + (int64_t)idxN * 32)[0]; nq1 = reinterpret_cast<const uint4*>(kf.D + (int64_t)idxN * 32)[1];
            nvalid = kfValid[idxN];
        }
        for (int ia = a0; ia < a1; ia++) {
            const int realIdxKF = __builtin_amdgcn_readfirstlane(idxN);
            const uint4 q0 = nq0, q1 = nq1;
            const bool valid = nvalid != 0;
            idxN = idxN2;
            idxN2 = ia + 2 < a1 ? (int)kf.feat[ia + 2] : 0;
            if (ia + 1 < a1) {
                nq0 = reinterpret_cast<const uint4*>(kf.D + (int64_t)idxN * 32)[0]; nq1 = reinterpret_cast<const uint4*>(kf.D + (int64_t)idxN * 32)[1];
                nvalid = kfValid[idxN];
            }
            if (!valid) continue;                                         // !pMP || pMP->isBad() (:208-213)
            unsigned b1key = 0xFFFFFFFFu, b2key = 0xFFFFFFFFu;
            if (inRegs) {
#pragma unroll
                for (int r = 0; r < BOW_R; r++) {
                    if (idxF[r] < 0 || (takenBits >> r) & 1u) continue;   // vpMapPointMatches[realIdxF] (:219-220)
                    const int dist = pg_hamming256(q0, q1, d0[r], d1[r]);
                    const unsigned key = ((unsigned)dist << 16) | (unsigned)(64 * r + lane);
                    if (key < b1key) { b2key = b1key; b1key = key; } else if (key < b2key) b2key = key;
                }
            } else {                                                      // a node with more frame features than the registers hold
                for (int k = lane; k < nb; k += 64) {
                    const int realIdxF = (int)fr.feat[b0 + k];
                    if (matchesOut[realIdxF] >= 0) continue;              // (this wave's own earlier writes: same lane, program order)
                    const unsigned key = ((unsigned)sfi_distance(q0, q1, fr.D + (int64_t)realIdxF * 32) << 16) | (unsigned)k;
                    if (key < b1key) { b2key = b1key; b1key = key; } else if (key < b2key) b2key = key;
                }
            }
            const unsigned w1 = wave_min_u32(b1key);
            if (w1 == 0xFFFFFFFFu || (int)(w1 >> 16) >= 256) continue;     // bestDist1 starts at 256
            const unsigned w2 = wave_min_u32(b1key == w1 ? b2key : b1key);
            const int bestDist1 = (int)(w1 >> 16);
            const int bestDist2 = (w2 != 0xFFFFFFFFu && (int)(w2 >> 16) < 256) ? (int)(w2 >> 16) : 256;
            if (bestDist1 <= TH_LOW && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {   // :233-235
                const int kbest = (int)(w1 & 0xFFFFu);
                if ((kbest & 63) == lane) {                              // the lane that holds the winner files it
                    int bestIdxF; float fang;
                    if (inRegs) {
                        const int r = kbest >> 6;
                        bestIdxF = idxF[0]; fang = ang[0];
#pragma unroll
                        for (int rr = 1; rr < BOW_R; rr++) if (r == rr) { bestIdxF = idxF[rr]; fang = ang[rr]; }
                        takenBits |= 1u << r;
                    } else {
                        bestIdxF = (int)fr.feat[b0 + kbest]; fang = fr.K[bestIdxF].angle;
                    }
                    matchesOut[bestIdxF] = realIdxKF;
                    binOut[bestIdxF] = (int8_t)(checkOrientation ? pg_rot_bin(kf.K[realIdxKF].angle, fang) : -1);    // :241-250
                }
                if (!inRegs) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the next feature's scan reads matchesOut from other lanes
            }
        }
    }
}

// ---- SearchByBoW(pKF1, pKF2, vpMatches12), src/ORBmatcher.cc:524-657 (loop closing) ----
// Differences from SearchByBoW(KeyFrame*, Frame&): bestDist1 < TH_LOW is strict (:600); KF2's side is masked by validity AND
// vbMatched2 (:578-582), and vbMatched2 is written only by an accepted match (:605); the output goes by KF1's feature.  A KF2 feature
// belongs to one vocabulary node, so vbMatched2 never crosses a node: one wave per (pair, common node) walks KF1's features of the
// node in FeatureVector order, KF2's features of it one per lane.  The finishing pass is k_match_finish over KF1's side with no drop
// mask: it histograms every bin >= 0 without looking at the matches, and this kernel writes a bin only together with its match and
// never clears either, so that is the histogram of the matches (:636-654).
struct PgKfBowBatch { PgFvBatch fv; const int32_t* kf1; const int32_t* kf2; const uint8_t* valid1; const uint8_t* valid2; };
#define KFBOW_WAVES 64           // waves per pair, each takes KF1's nodes a = wave, wave + 64, ...

__global__ __launch_bounds__(64) void k_bow_keyframes(PgKfBowBatch B, float nnratio, int checkOrientation, int32_t* __restrict__ m12,
                                                      int8_t* __restrict__ bins, uint8_t* matched2)
{
    const int p = blockIdx.y, cap = B.fv.cap, lane = threadIdx.x;
    const int f1 = B.kf1[p], f2 = B.kf2[p];
    PgFvView v1 = pg_fv_view(B.fv, f1), v2 = pg_fv_view(B.fv, f2);
    // the batched form trusts its FeatureVectors: it only clamps the counts here and the nodes' starts below
    v1.nfv = min(max(v1.nfv, 0), cap); v2.nfv = min(max(v2.nfv, 0), cap);
    const int n1 = min(max(B.fv.n[f1], 0), cap), n2 = min(max(B.fv.n[f2], 0), cap);
    const int64_t row = (int64_t)p * cap;
    for (int a = blockIdx.x; a < v1.nfv; a += KFBOW_WAVES) {
        const int lo = pg_fv_find_node(v2, v1.node[a]);                      // KF2's entry of the same node
        if (lo < 0) continue;
        const int a0 = max(v1.start[a], 0), a1 = min(v1.start[a + 1], cap), b0 = max(v2.start[lo], 0), b1 = min(v2.start[lo + 1], cap);
        for (int ia = a0; ia < a1; ia++) {                                    // KF1's features of the node, in order (:556)
            const int idx1 = (int)v1.feat[ia];
            if ((unsigned)idx1 >= (unsigned)n1 || !B.valid1[row + idx1]) continue;     // !pMP1 || pMP1->isBad() (:560-564)
            const uint4 q0 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idx1 * 32)[0];
            const uint4 q1 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idx1 * 32)[1];
            unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;                      // the lane's two smallest (distance << 16 | list position)
            for (int k = lane; b0 + k < b1; k += 64) {
                const int idx2 = (int)v2.feat[b0 + k];
                if ((unsigned)idx2 >= (unsigned)n2) continue;
                if (matched2[row + idx2] || !B.valid2[row + idx2]) continue;  // vbMatched2[idx2] || !pMP2 || pMP2->isBad() (:578-582)
                const unsigned key = ((unsigned)sfi_distance(q0, q1, v2.D + (int64_t)idx2 * 32) << 16) | (unsigned)k;
                if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
            }
            const unsigned w1 = wave_min_u32(k1);
            if (w1 == 0xFFFFFFFFu) continue;
            const unsigned w2 = wave_min_u32(k1 == w1 ? k2 : k1);
            const int bestDist1 = (int)(w1 >> 16), bestDist2 = w2 == 0xFFFFFFFFu ? 256 : (int)(w2 >> 16);
            if (bestDist1 < TH_LOW && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {     // :600-602
                const int kbest = (int)(w1 & 0xFFFFu);
                if ((kbest & 63) == lane) {
                    const int idx2 = (int)v2.feat[b0 + kbest];
                    m12[row + idx1] = idx2;                                   // :604-605
                    matched2[row + idx2] = 1;
                    bins[row + idx1] = (int8_t)(checkOrientation ? pg_rot_bin(v1.K[idx1].angle, v2.K[idx2].angle) : -1);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the next feature's scan reads matched2 from other lanes
            }
        }
    }
}

// after the nodes: count the matches of a pair and apply the rotation histogram.  The output side of pair p is frame
// pairSide[p] (SearchByBoW: the frame; SearchByBoW(KF, KF) and SearchForTriangulation: key frame 1).  drop ([npairs][cap] or null) clears the entries
// it marks before anything is counted: SearchForTriangulation's "KF1 keypoint already has a map point" (ORBmatcher.cc:701-705).
__global__ __launch_bounds__(64) void k_match_finish(const int32_t* __restrict__ pairSide, const int32_t* __restrict__ nper, int cap,
                                                     const uint8_t* __restrict__ drop, int checkOrientation, int32_t* __restrict__ matchesOut,
                                                     const int8_t* __restrict__ binIn, int32_t* __restrict__ nmatchesOut)
{
    const int p = blockIdx.x, nf = min(nper[pairSide[p]], cap), lane = threadIdx.x;
    matchesOut += (int64_t)p * cap; binIn += (int64_t)p * cap; nmatchesOut += p;
    if (drop) drop += (int64_t)p * cap;
    int nmatches = 0;
    for (int i = lane; i < nf; i += 64) {
        int m = matchesOut[i];
        if (m >= 0 && drop && drop[i]) { matchesOut[i] = -1; m = -1; }
        nmatches += m >= 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nmatches += __shfl_xor(nmatches, d);
    const int8_t* rotBin = binIn;
    int32_t* asg = matchesOut;
    if (checkOrientation) {                                               // :256-277
        // the 30 bin sizes: lanes stride over the features, one LDS atomic each (every lane walking all nf bins by itself, a dependent
        // byte load per feature, was 90 of this kernel's 93 us at 2 000 features)
        __shared__ int hist[64];
        hist[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < nf; i += 64) { const int bb = rotBin[i]; if (bb >= 0 && !(drop && drop[i])) atomicAdd(&hist[bb & 63], 1); }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int h = hist[lane];
        int ind1, ind2, ind3;
        pg_three_maxima([&](int i) { return __shfl(h, i); }, ind1, ind2, ind3);
        int removed = 0;
        for (int i = lane; i < nf; i += 64) {
            const int bb = rotBin[i];
            if (bb >= 0 && bb != ind1 && bb != ind2 && bb != ind3 && asg[i] >= 0) { asg[i] = -1; removed++; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) removed += __shfl_xor(removed, d);
        nmatches -= removed;
    }
    if (lane == 0) *nmatchesOut = nmatches;
}

// ---- SearchForTriangulation(KF1, KF2, F12, vMatchedPairs, bOnlyStereo = false), src/ORBmatcher.cc:659-825, 142-159 ----
// The same node walk as SearchByBoW, from KF1's side, with no order dependence at all: vbMatched2 (:679) is read (:727) but never
// set, so every KF1 keypoint is decided on its own and two of them may take the same KF2 keypoint.  One wave per (pair, KF1
// node): KF2's keypoints of the node one per lane and held in registers together with what does not depend on KF1 -- the
// has_point2 mask and the epipole test (:745-751) fold into "no candidate" -- and KF1's keypoints walked with their descriptors
// prefetched.  Per KF1 keypoint a candidate passes on dist <= TH_LOW and the epipolar test; bestDist only moves on a passing
// candidate (:753-757), so the reference keeps the LAST passing candidate of the smallest distance: a wave minimum on
// (dist << 16 | 0xFFFF - list position).  KF1's own mask (:701-705) is applied by k_match_finish, so this pass depends only on
// (KF1, KF2, F12, epipole, has_point2).
#define TRI_R 4                  // KF2 keypoints per lane held in registers: nodes of up to 256 KF2 keypoints
#define TRI_WAVES 64             // waves per pair, each takes the KF1 nodes a = wave, wave + 64, ...

// the KF1-independent part of a candidate: has_point2 (:724-728) and the epipole test (:745-751, float; a NaN / infinite
// epipole never rejects)
__device__ __forceinline__ bool tri_candidate(const pgorb_keypoint& kp2, bool hasPoint, float ex, float ey, const float* epiTh)
{
    if (hasPoint) return false;
    const float dx = __fsub_rn(ex, kp2.x), dy = __fsub_rn(ey, kp2.y);
    return !(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < epiTh[min((unsigned)kp2.octave, (unsigned)PG_MAXL)]);
}
// CheckDistEpipolarLine (:142-159) past the den == 0 test: num = a*x2 + b*y2 + c, dsqr = num*num/den in float, compared in double
__device__ __forceinline__ bool tri_on_line(float la, float lb, float lc, float den, float x2, float y2, double th)
{
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, x2), __fmul_rn(lb, y2)), lc);
    return (double)__fdiv_rn(__fmul_rn(num, num), den) < th;
}

__global__ __launch_bounds__(64) void k_search_for_triangulation(PgTriBatch T, int checkOrientation, int32_t* __restrict__ matchesOut,
                                                                 int8_t* __restrict__ binOut)
{
    const int p = blockIdx.y, cap = T.fv.cap, lane = threadIdx.x;
    __shared__ float sEpi[PG_MAXL + 1];
    __shared__ double sLine[PG_MAXL + 1];
    __shared__ float sGeo[11];                                            // F12 (row-major), ex, ey
    if (lane <= PG_MAXL) { sEpi[lane] = T.epiTh[lane]; sLine[lane] = T.lineTh[lane]; }
    if (lane < 9) sGeo[lane] = T.F12[(int64_t)p * 9 + lane];
    else if (lane < 11) sGeo[lane] = T.epipole[2 * p + lane - 9];
    __syncthreads();
    const PgFvView v1 = pg_fv_view(T.fv, T.pairKF1[p]), v2 = pg_fv_view(T.fv, T.pairKF2[p]);
    const uint8_t* __restrict__ has2 = T.hasPoint2 + (int64_t)p * cap;
    const float ex = sGeo[9], ey = sGeo[10];
    matchesOut += (int64_t)p * cap; binOut += (int64_t)p * cap;
    for (int a = blockIdx.x; a < v1.nfv; a += TRI_WAVES) {
        const int lo = pg_fv_find_node(v2, v1.node[a]);                  // KF2's entry of the same node
        if (lo < 0) continue;
        const int a0 = v1.start[a], a1 = v1.start[a + 1], b0 = v2.start[lo], b1 = v2.start[lo + 1], nb = b1 - b0;
        const bool inRegs = nb <= 64 * TRI_R;
        // KF2's keypoints of the node: lane holds list positions k = lane, lane + 64, ...; idx2 = -1: no candidate for any KF1 keypoint
        uint4 d0[TRI_R], d1[TRI_R]; float x2[TRI_R], y2[TRI_R], ang2[TRI_R]; double th2[TRI_R]; int idx2[TRI_R];
#pragma unroll
        for (int r = 0; r < TRI_R; r++) {
            const int k = 64 * r + lane;
            idx2[r] = -1; x2[r] = y2[r] = ang2[r] = 0.f; th2[r] = 0.0; d0[r] = make_uint4(0, 0, 0, 0); d1[r] = d0[r];
            if (inRegs && k < nb) {
                const int j = (int)v2.feat[b0 + k];
                const pgorb_keypoint kp2 = v2.K[j];
                if (tri_candidate(kp2, has2[j] != 0, ex, ey, sEpi)) {
                    idx2[r] = j;
                    d0[r] = reinterpret_cast<const uint4*>(v2.D + (int64_t)j * 32)[0];
                    d1[r] = reinterpret_cast<const uint4*>(v2.D + (int64_t)j * 32)[1];
                    x2[r] = kp2.x; y2[r] = kp2.y; ang2[r] = kp2.angle;
                    th2[r] = sLine[min((unsigned)kp2.octave, (unsigned)PG_MAXL)];
                }
            }
        }
        // KF1's keypoints of the node: the index two iterations ahead, descriptor and keypoint one ahead (all lanes load the same
        // addresses); nothing inside the loop depends on an earlier KF1 keypoint
        int idxN = a0 < a1 ? (int)v1.feat[a0] : 0, idxN2 = a0 + 1 < a1 ? (int)v1.feat[a0 + 1] : 0;
        uint4 nq0 = make_uint4(0, 0, 0, 0), nq1 = nq0;
        float nx = 0.f, ny = 0.f, nang = 0.f;
        if (a0 < a1) {
            nq0 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idxN * 32)[0]; nq1 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idxN * 32)[1];
            nx = v1.K[idxN].x; ny = v1.K[idxN].y; nang = v1.K[idxN].angle;
        }
        for (int ia = a0; ia < a1; ia++) {
            const int idx1 = __builtin_amdgcn_readfirstlane(idxN);
            const uint4 q0 = nq0, q1 = nq1;
            const float x1 = nx, y1 = ny, ang1 = nang;
            idxN = idxN2;
            idxN2 = ia + 2 < a1 ? (int)v1.feat[ia + 2] : 0;
            if (ia + 1 < a1) {
                nq0 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idxN * 32)[0]; nq1 = reinterpret_cast<const uint4*>(v1.D + (int64_t)idxN * 32)[1];
                nx = v1.K[idxN].x; ny = v1.K[idxN].y; nang = v1.K[idxN].angle;
            }
            // the epipolar line of kp1 in KF2, l = x1'F12 = [a b c] (:145-147), and den = a*a + b*b (:151); F12.at<float>(r, c) =
            // sGeo[3 * r + c], read from the LDS per keypoint (held in SGPRs across the loop they overflowed the SGPR file)
            const float F00 = sGeo[0], F01 = sGeo[1], F02 = sGeo[2], F10 = sGeo[3], F11 = sGeo[4], F12 = sGeo[5], F20 = sGeo[6], F21 = sGeo[7], F22 = sGeo[8];
            const float la = __fadd_rn(__fadd_rn(__fmul_rn(x1, F00), __fmul_rn(y1, F10)), F20);
            const float lb = __fadd_rn(__fadd_rn(__fmul_rn(x1, F01), __fmul_rn(y1, F11)), F21);
            const float lc = __fadd_rn(__fadd_rn(__fmul_rn(x1, F02), __fmul_rn(y1, F12)), F22);
            const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
            if (den == 0.0f) continue;                                    // every candidate fails CheckDistEpipolarLine (:153-154)
            unsigned best = 0xFFFFFFFFu;
            if (inRegs) {
#pragma unroll
                for (int r = 0; r < TRI_R; r++) {                       // (no branches: every slot is evaluated, empty ones drop out)
                    const int dist = pg_hamming256(q0, q1, d0[r], d1[r]);
                    const bool pass = idx2[r] >= 0 && dist <= TH_LOW && tri_on_line(la, lb, lc, den, x2[r], y2[r], th2[r]);
                    best = min(best, pass ? ((unsigned)dist << 16) | (unsigned)(0xFFFF - (64 * r + lane)) : 0xFFFFFFFFu);
                }
            } else {                                                      // a node with more KF2 keypoints than the registers hold
                for (int k = lane; k < nb; k += 64) {
                    const int j = (int)v2.feat[b0 + k];
                    const pgorb_keypoint kp2 = v2.K[j];
                    if (!tri_candidate(kp2, has2[j] != 0, ex, ey, sEpi)) continue;
                    const int dist = sfi_distance(q0, q1, v2.D + (int64_t)j * 32);
                    if (dist > TH_LOW || !tri_on_line(la, lb, lc, den, kp2.x, kp2.y, sLine[min((unsigned)kp2.octave, (unsigned)PG_MAXL)])) continue;
                    best = min(best, ((unsigned)dist << 16) | (unsigned)(0xFFFF - k));
                }
            }
            const unsigned w = wave_min_u32(best);
            if (w == 0xFFFFFFFFu) continue;
            const int kbest = 0xFFFF - (int)(w & 0xFFFFu);
            if ((kbest & 63) == lane) {                                   // the lane that holds the winner files it (:758-777)
                int j; float a2;
                if (inRegs) {
                    const int r = kbest >> 6;
                    j = idx2[0]; a2 = ang2[0];
#pragma unroll
                    for (int rr = 1; rr < TRI_R; rr++) if (r == rr) { j = idx2[rr]; a2 = ang2[rr]; }
                } else {
                    j = (int)v2.feat[b0 + kbest]; a2 = v2.K[j].angle;
                }
                matchesOut[idx1] = j;
                binOut[idx1] = (int8_t)(checkOrientation ? pg_rot_bin(ang1, a2) : -1);
            }
        }
    }
}

// the launches of a BoW-node matcher on `stream`: clear the outputs, the node pass (nodePass launches it), the finishing pass over
// the pairs' output side; bins = [npairs][cap] i8 scratch.  The caller asks hipGetLastError under its node kernel's name.
template <class F> static int pg_node_match_launch(pgorb_ctx* c, int npairs, int cap, const int32_t* d_pair_side, const int32_t* d_n,
                                                   const uint8_t* d_drop, int check_orientation, int32_t* d_matches, int8_t* bins,
                                                   int32_t* d_nmatches, hipStream_t stream, F&& nodePass)
{
    if (hipMemsetAsync(d_matches, 0xFF, (size_t)npairs * cap * 4, stream) != hipSuccess ||
        hipMemsetAsync(bins, 0xFF, (size_t)npairs * cap, stream) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    nodePass();
    hipLaunchKernelGGL(k_match_finish, dim3(npairs), dim3(64), 0, stream, d_pair_side, d_n, cap, d_drop, check_orientation, d_matches,
                       (const int8_t*)bins, d_nmatches);
    return 0;
}

int pg_tri_launch(pgorb_ctx* c, PgTriBatch T, int npairs, const uint8_t* d_has_point1, int check_orientation, int32_t* d_matches12,
                  int8_t* bins, int32_t* d_nmatches, hipStream_t stream)
{
    // the per-octave thresholds exactly as the reference forms them: 100*float (int promoted to float) and 3.84*double(float)
    float sf[PG_MAXL + 1] = {0}, s2[PG_MAXL + 1] = {0};
    pgorb_scale_tables(c, sf, nullptr, s2, nullptr);
    for (int l = 0; l <= PG_MAXL; l++) { T.epiTh[l] = 100.0f * sf[l]; T.lineTh[l] = 3.84 * (double)s2[l]; }
    const int rc = pg_node_match_launch(c, npairs, T.fv.cap, T.pairKF1, T.fv.n, d_has_point1, check_orientation, d_matches12, bins, d_nmatches, stream, [&] {
        hipLaunchKernelGGL(k_search_for_triangulation, dim3(TRI_WAVES, npairs), dim3(64), 0, stream, T, check_orientation, d_matches12, bins); });
    if (rc) return rc;
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_search_for_triangulation launch failed");
    return 0;
}

bool pg_fv_ok(const int32_t* start, const uint32_t* feat, int nfv, int n)
{
    if (nfv > n || start[0] != 0 || start[nfv] > n) return false;
    for (int a = 0; a < nfv; a++) if (start[a + 1] < start[a]) return false;
    for (int i = 0; i < start[nfv]; i++) if (feat[i] >= (uint32_t)n) return false;
    return true;
}

PgFvPack::PgFvPack(PgHostCall& s, const PgFvFrame* f, int nframes) : nframes(nframes), cap(1)
{
    for (int k = 0; k < nframes; k++) cap = std::max(cap, f[k].n);
    const size_t slots = (size_t)nframes * cap, nf4 = (size_t)nframes * 4;
    K = s.region(PG_UP, slots * sizeof(pgorb_keypoint)); D = s.region(PG_UP, slots * 32); H = s.region(PG_UP, slots);
    N = s.region(PG_UP, nf4); FN = s.region(PG_UP, slots * 4); FS = s.region(PG_UP, (slots + nframes) * 4); FF = s.region(PG_UP, slots * 4);
    NF = s.region(PG_UP, nf4); P = s.region(PG_UP, nf4);
}
void PgFvPack::pack(PgHostCall& s, const PgFvFrame* f) const
{
    const size_t kb = sizeof(pgorb_keypoint);
    for (int k = 0; k < nframes; k++) {
        const PgFvFrame& F = f[k];
        const size_t n = F.n, m = F.nfv, slot = (size_t)k * cap;
        s.host<int32_t>(N)[k] = F.n; s.host<int32_t>(NF)[k] = F.nfv; s.host<int32_t>(P)[k] = k;
        s.put(K, F.kps, n * kb, slot * kb, cap * kb);
        if (!F.kps) for (size_t i = 0; i < n; i++) s.host<pgorb_keypoint>(K)[slot + i].angle = F.angle[i];
        s.put(D, F.desc, n * 32, slot * 32, cap * 32);
        s.put(H, F.mask, n, slot, cap);
        s.put(FN, F.node, m * 4, slot * 4, cap * 4);
        s.put(FS, F.start, (m + 1) * 4, (slot + k) * 4, (cap + 1) * 4);
        s.put(FF, F.feat, (size_t)F.start[m] * 4, slot * 4, cap * 4);
    }
}

extern "C" {

// single pair through host buffers: the pair becomes a two-frame batch (key frame = frame 0, frame = frame 1)
int pgorb_search_by_bow(pgorb_ctx* c, const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_point_valid, int nkf,
                        const uint32_t* kf_fv_node, const int32_t* kf_fv_start, const uint32_t* kf_fv_feat, int kf_nfv,
                        const uint8_t* f_desc, const float* f_angle, int nf, const uint32_t* f_fv_node,
                        const int32_t* f_fv_start, const uint32_t* f_fv_feat, int f_nfv, float nnratio,
                        int check_orientation, int32_t* matches)
{
    if (!c) return PGORB_E_ARG;
    if (nkf < 0 || nf < 0 || kf_nfv < 0 || f_nfv < 0 || (nf && !matches) ||
        (nkf && (!kf_desc || !kf_angle || !kf_point_valid)) || (nf && (!f_desc || !f_angle)) ||
        (kf_nfv && (!kf_fv_node || !kf_fv_start || !kf_fv_feat)) || (f_nfv && (!f_fv_node || !f_fv_start || !f_fv_feat)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow");
    for (int i = 0; i < nf; i++) matches[i] = -1;
    if (!nkf || !nf || !kf_nfv || !f_nfv) return 0;
    if (nf > 16000 || nkf > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (!pg_fv_ok(kf_fv_start, kf_fv_feat, kf_nfv, nkf) || !pg_fv_ok(f_fv_start, f_fv_feat, f_nfv, nf))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow: FeatureVector names more features than the frame has");
    const PgFvFrame f[2] = {{nullptr, kf_angle, kf_desc, kf_point_valid, nkf, kf_fv_node, kf_fv_start, kf_fv_feat, kf_nfv},
                            {nullptr, f_angle, f_desc, nullptr, nf, f_fv_node, f_fv_start, f_fv_feat, f_nfv}};
    PgHostCall s(c);
    const PgFvPack p(s, f, 2);
    const size_t oM = s.region(PG_DOWN, (size_t)p.cap * 4), oNM = s.region(PG_DOWN, 4);
    int rc = s.begin();
    if (rc) return rc;
    p.pack(s, f);
    if ((rc = s.run([&] {
            return pgorb_search_by_bow_batch_device(c, s.dev<pgorb_keypoint>(p.K), s.dev(p.D), s.dev<int32_t>(p.N), p.cap, s.dev<uint32_t>(p.FN),
                                                    s.dev<int32_t>(p.FS), s.dev<uint32_t>(p.FF), s.dev<int32_t>(p.NF), s.dev<int32_t>(p.P),
                                                    s.dev<int32_t>(p.P) + 1, 1, s.dev(p.H), nnratio, check_orientation, s.dev<int32_t>(oM),
                                                    s.dev<int32_t>(oNM), nullptr); }))) return rc;
    memcpy(matches, s.host(oM), (size_t)nf * 4);
    return *s.host<int32_t>(oNM);
}

int pgorb_feature_vectors_batch_device(pgorb_ctx* c, const uint32_t* d_node, const int32_t* d_n, int nframes, int cap,
                                       uint32_t* d_fv_node, int32_t* d_fv_start, uint32_t* d_fv_feat, int32_t* d_nfv, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_node || !d_n || nframes < 1 || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_feature_vectors_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    static const bool counting = getenv("PGORB_FV_COUNTING") != nullptr;      // (A / B switch: the O(n^2) counting form for every size)
    if (cap <= FV_T * FV_IPT && !counting) {
        const size_t ldsS = (size_t)2 * FV_T * FV_IPT * 8 + (2 * FV_T / 64 + 2) * 4;       // two key buffers + the wave totals
        if (!pg_raise_lds<k_feature_vectors_sorted>(c, ldsS)) return pg_ctx_fail(c, PGORB_E_LIMIT, "feature vector scratch exceeds the LDS");
        hipLaunchKernelGGL(k_feature_vectors_sorted, dim3(nframes), dim3(FV_T), ldsS, (hipStream_t)stream, d_node, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv);
        if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_feature_vectors_sorted launch failed");
        return 0;
    }
    const size_t lds = (size_t)cap * 8 + 1025 * 4;
    if (!pg_raise_lds<k_feature_vectors>(c, lds)) return pg_ctx_fail(c, PGORB_E_LIMIT, "feature vector scratch exceeds the LDS");
    hipLaunchKernelGGL(k_feature_vectors, dim3(nframes), dim3(1024), lds, (hipStream_t)stream, d_node, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_feature_vectors launch failed");
    return 0;
}

int pgorb_search_by_bow_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                     const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
                                     const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs, const uint8_t* d_kf_point_valid,
                                     float nnratio, int check_orientation, int32_t* d_matches, int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv || npairs < 0 ||
        (npairs && (!d_pair_kf || !d_pair_f || !d_kf_point_valid || !d_matches || !d_nmatches)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    // scratch: the rotation bin of every matched frame feature [npairs][cap] i8
    void* scratch;
    int rcs = pg_ctx_scratch(c, (size_t)npairs * cap + 256, (hipStream_t)stream, &scratch);
    if (rcs) return rcs;
    int8_t* bins = (int8_t*)scratch;
    const PgBowBatch B = {{d_kps, d_desc, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv}, d_pair_kf, d_pair_f, d_kf_point_valid};
    rcs = pg_node_match_launch(c, npairs, cap, d_pair_f, d_n, nullptr, check_orientation, d_matches, bins, d_nmatches, (hipStream_t)stream, [&] {
        hipLaunchKernelGGL(k_search_by_bow, dim3(BOW_WAVES, npairs), dim3(64), 0, (hipStream_t)stream, B, nnratio, check_orientation, d_matches, bins); });
    if (rcs) return rcs;
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_search_by_bow launch failed");
    return pg_ctx_scratch_done(c, (hipStream_t)stream);
}

int pgorb_search_by_bow_keyframes_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                               const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat,
                                               const int32_t* d_nfv, const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs,
                                               const uint8_t* d_point_valid1, const uint8_t* d_point_valid2, float nnratio,
                                               int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv || npairs < 0 ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_point_valid1 || !d_point_valid2 || !d_matches12 || !d_nmatches)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow_keyframes_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const size_t rb = (size_t)npairs * cap;                                  // the rotation bins (i8) and vbMatched2 (u8) of every pair
    PgCarve cv;
    const size_t oBins = cv.take(rb), oM2 = cv.take(rb);
    void* scr;
    int rc = pg_ctx_scratch(c, cv.o, s, &scr);
    if (rc) return rc;
    int8_t* bins = (int8_t*)scr + oBins;
    uint8_t* matched2 = (uint8_t*)scr + oM2;
    const PgKfBowBatch B = {{d_kps, d_desc, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv}, d_pair_kf1, d_pair_kf2, d_point_valid1,
                            d_point_valid2};
    bool cleared = false;
    rc = pg_node_match_launch(c, npairs, cap, d_pair_kf1, d_n, nullptr, check_orientation, d_matches12, bins, d_nmatches, s, [&] {
        if ((cleared = hipMemsetAsync(matched2, 0, rb, s) == hipSuccess))
            hipLaunchKernelGGL(k_bow_keyframes, dim3(KFBOW_WAVES, (unsigned)npairs), dim3(64), 0, s, B, nnratio, check_orientation, d_matches12, bins, matched2); });
    if (rc) return rc;
    if (!cleared) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_bow_keyframes launch failed");
    return pg_ctx_scratch_done(c, s);
}

// single pair through host buffers: a two-frame batch (KF1 = frame 0, KF2 = frame 1); the FeatureVectors are checked here
int pgorb_search_by_bow_keyframes(pgorb_ctx* c, const uint8_t* desc1, const float* angle1, const uint8_t* point_valid1, int n1,
                                  const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1,
                                  const uint8_t* desc2, const float* angle2, const uint8_t* point_valid2, int n2,
                                  const uint32_t* fv2_node, const int32_t* fv2_start, const uint32_t* fv2_feat, int nfv2,
                                  float nnratio, int check_orientation, int32_t* matches12)
{
    if (!c) return PGORB_E_ARG;
    if (n1 < 0 || n2 < 0 || nfv1 < 0 || nfv2 < 0 || (n1 && !matches12) || (n1 && (!desc1 || !angle1 || !point_valid1)) ||
        (n2 && (!desc2 || !angle2 || !point_valid2)) || (nfv1 && (!fv1_node || !fv1_start || !fv1_feat)) ||
        (nfv2 && (!fv2_node || !fv2_start || !fv2_feat)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_by_bow_keyframes");
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (!n1 || !n2 || !nfv1 || !nfv2) return 0;
    if (n1 > 16000 || n2 > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (!pg_fv_ok(fv1_start, fv1_feat, nfv1, n1) || !pg_fv_ok(fv2_start, fv2_feat, nfv2, n2))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: FeatureVector names more features than the key frame has");
    for (int a = 1; a < nfv1; a++) if (!(fv1_node[a - 1] < fv1_node[a])) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: node ids must ascend");
    for (int a = 1; a < nfv2; a++) if (!(fv2_node[a - 1] < fv2_node[a])) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_by_bow_keyframes: node ids must ascend");
    const PgFvFrame f[2] = {{nullptr, angle1, desc1, point_valid1, n1, fv1_node, fv1_start, fv1_feat, nfv1},
                            {nullptr, angle2, desc2, point_valid2, n2, fv2_node, fv2_start, fv2_feat, nfv2}};
    PgHostCall hc(c);
    const PgFvPack pk(hc, f, 2);
    const size_t oM = hc.region(PG_DOWN, (size_t)pk.cap * 4), oNM = hc.region(PG_DOWN, 4);
    int rc = hc.begin();
    if (rc) return rc;
    pk.pack(hc, f);
    if ((rc = hc.run([&] {
            return pgorb_search_by_bow_keyframes_batch_device(c, hc.dev<pgorb_keypoint>(pk.K), hc.dev(pk.D), hc.dev<int32_t>(pk.N), pk.cap,
                                                              hc.dev<uint32_t>(pk.FN), hc.dev<int32_t>(pk.FS), hc.dev<uint32_t>(pk.FF),
                                                              hc.dev<int32_t>(pk.NF), hc.dev<int32_t>(pk.P), hc.dev<int32_t>(pk.P) + 1, 1,
                                                              hc.dev(pk.H), hc.dev(pk.H) + pk.cap, nnratio, check_orientation,
                                                              hc.dev<int32_t>(oM), hc.dev<int32_t>(oNM), nullptr); }))) return rc;
    memcpy(matches12, hc.host(oM), (size_t)n1 * 4);
    return *hc.host<int32_t>(oNM);
}

// single pair through host buffers: the pair becomes a two-frame batch (KF1 = frame 0, KF2 = frame 1)
int pgorb_search_for_triangulation(pgorb_ctx* c, const pgorb_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_point1, int n1,
                                   const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1,
                                   const pgorb_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_point2, int n2,
                                   const uint32_t* fv2_node, const int32_t* fv2_start, const uint32_t* fv2_feat, int nfv2,
                                   const float F12[9], float ex, float ey, int check_orientation, int32_t* matches12)
{
    if (!c) return PGORB_E_ARG;
    if (n1 < 0 || n2 < 0 || nfv1 < 0 || nfv2 < 0 || !F12 || (n1 && !matches12) || (n1 && (!kps1 || !desc1)) || (n2 && (!kps2 || !desc2)) ||
        !fv1_start || !fv2_start || (nfv1 && (!fv1_node || !fv1_feat)) || (nfv2 && (!fv2_node || !fv2_feat)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_for_triangulation");
    if (n1 > 16000 || n2 > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (!pg_fv_ok(fv1_start, fv1_feat, nfv1, n1) || !pg_fv_ok(fv2_start, fv2_feat, nfv2, n2))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_search_for_triangulation: FeatureVector names more features than the key frame has");
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (!n1 || !n2 || !nfv1 || !nfv2) return 0;
    const PgFvFrame f[2] = {{kps1, nullptr, desc1, has_point1, n1, fv1_node, fv1_start, fv1_feat, nfv1},
                            {kps2, nullptr, desc2, has_point2, n2, fv2_node, fv2_start, fv2_feat, nfv2}};
    PgHostCall s(c);
    const PgFvPack p(s, f, 2);
    const size_t oF = s.region(PG_UP, 9 * 4), oE = s.region(PG_UP, 8), oM = s.region(PG_DOWN, (size_t)p.cap * 4), oNM = s.region(PG_DOWN, 4);
    int rc = s.begin();
    if (rc) return rc;
    p.pack(s, f);
    const float ep[2] = {ex, ey};
    s.put(oF, F12, 9 * 4); s.put(oE, ep, 8);
    if ((rc = s.run([&] {
            return pgorb_search_for_triangulation_batch_device(c, s.dev<pgorb_keypoint>(p.K), s.dev(p.D), s.dev<int32_t>(p.N), p.cap,
                                                               s.dev<uint32_t>(p.FN), s.dev<int32_t>(p.FS), s.dev<uint32_t>(p.FF),
                                                               s.dev<int32_t>(p.NF), s.dev<int32_t>(p.P), s.dev<int32_t>(p.P) + 1, 1,
                                                               s.dev<float>(oF), s.dev<float>(oE), s.dev(p.H), s.dev(p.H) + p.cap,
                                                               check_orientation, s.dev<int32_t>(oM), s.dev<int32_t>(oNM), nullptr); }))) return rc;
    memcpy(matches12, s.host(oM), (size_t)n1 * 4);
    return *s.host<int32_t>(oNM);
}

int pgorb_search_for_triangulation_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                                const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
                                                const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs, const float* d_F12,
                                                const float* d_epipole, const uint8_t* d_has_point1, const uint8_t* d_has_point2,
                                                int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_desc || !d_n || cap < 1 || !d_fv_node || !d_fv_start || !d_fv_feat || !d_nfv || npairs < 0 ||
        (npairs && (!d_pair_kf1 || !d_pair_kf2 || !d_F12 || !d_epipole || !d_matches12 || !d_nmatches)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_search_for_triangulation_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    PgTriBatch T = {{d_kps, d_desc, d_n, cap, d_fv_node, d_fv_start, d_fv_feat, d_nfv}, d_pair_kf1, d_pair_kf2, d_F12, d_epipole, d_has_point2, {0}, {0}};
    // scratch: the rotation bin of every matched KF1 keypoint [npairs][cap] i8, then (no d_has_point2) an all-zero mask
    void* scratch;
    PgCarve cv;
    const size_t oBins = cv.take((size_t)npairs * cap), oHas = cv.take(d_has_point2 ? 0 : (size_t)npairs * cap);
    int rcs = pg_ctx_scratch(c, cv.o, (hipStream_t)stream, &scratch);
    if (rcs) return rcs;
    int8_t* bins = (int8_t*)scratch + oBins;
    if (!d_has_point2) {
        T.hasPoint2 = (const uint8_t*)scratch + oHas;
        if (hipMemsetAsync((uint8_t*)scratch + oHas, 0, (size_t)npairs * cap, (hipStream_t)stream) != hipSuccess)
            return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    }
    if ((rcs = pg_tri_launch(c, T, npairs, d_has_point1, check_orientation, d_matches12, bins, d_nmatches, (hipStream_t)stream)))
        return rcs;
    return pg_ctx_scratch_done(c, (hipStream_t)stream);
}

}  // extern "C"
