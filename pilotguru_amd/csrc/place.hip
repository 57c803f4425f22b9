// place.hip -- place recognition on gfx950: BowVectors on the device, batched L1 scores, and the candidate queries of
// KeyFrameDatabase (DetectRelocalizationCandidates, DetectLoopCandidates).
//
// Restates (thirdparty/orb-slam2 and its Thirdparty/DBoW2):
//   TemplatedVocabulary::transform (BowVector)    DBoW2/TemplatedVocabulary.h:1126-1194, BowVector.cpp:34-84
//   L1Scoring::score                              DBoW2/ScoringObject.cpp:23-60
//   KeyFrameDatabase::add / erase                 src/KeyFrameDatabase.cc:53-59, 61-80
//   KeyFrameDatabase::DetectLoopCandidates        src/KeyFrameDatabase.cc:89-210
//   KeyFrameDatabase::DetectRelocalizationCandidates  src/KeyFrameDatabase.cc:212-310
//
// A query decomposes exactly into two passes (the argument is in pgorb.h and DESIGN.md section 4):
//   k_place_overlap  one wave per (query, key frame): lanes take 64-word slices of the query's sorted ids and binary-search the
//                    key frame's; the common terms are taken in word order from the ballot and added into ONE running double
//                    (L1Scoring::score's sum); out come the number of common words, the smallest common word and the score.
//   k_place_decide   one workgroup per query: maxCommonWords, the (int)(max * 0.8f) threshold, the stored scores, then -- each
//                    scored key frame on its own, because an entry of lScoreAndMatch reads only stored scores -- the float
//                    accumulation over the first 10 covisible key frames with its pBestKF; the maximum, the retention, and the
//                    emitted key frames ordered by the first retained entry that names them (atomicMin of the entry's place in
//                    the sharing list = (smallest common word, add index)), ranked by counting.
// Every (query, key frame) row lives in a global slab (40 bytes per pair), so no list is bounded by the LDS.
#include "match_common.h"

#include <algorithm>
#include <string>

#define PL_T 1024
#define PL_NEIGH 10                       // GetBestCovisibilityKeyFrames(10)
#define PL_MAX_FRAMES 65536               // a key frame index is 16 bits of the ordering keys
#define BV_T 1024
#define BV_MAX 8192                       // features per frame of k_bow_vectors (BV_T threads x 8 consecutive ranks)

struct PgBowTable { const uint32_t* id; const double* val; const int32_t* n; int nframes, cap; };

__device__ __forceinline__ int pl_len(const PgBowTable& T, int f) { return ((unsigned)f < (unsigned)T.nframes) ? min(max(T.n[f], 0), T.cap) : 0; }

// One wave: the words lists A and B share (both ascending, no repeats).  count = their number, first = the smallest, sum =
// the running double sum of fabs(a - b) - fabs(a) - fabs(b) in ascending word order (ScoringObject.cpp:34-52), from 0.
__device__ __forceinline__ void pl_overlap(const uint32_t* __restrict__ idA, const double* __restrict__ vA, int nA,
                                           const uint32_t* __restrict__ idB, const double* __restrict__ vB, int nB, int lane,
                                           int& count, uint32_t& first, double& sum)
{
    count = 0; first = 0u; sum = 0.0;
    if (nB <= 0) return;
    for (int base = 0; base < nA; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double term = 0.0;
        if (i < nA) {
            const uint32_t w = idA[i];
            int lo = 0, hi = nB;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (idB[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nB && idB[lo] == w) {
                hit = true;
                const double a = vA[i], b = vB[lo];
                term = __dsub_rn(__dsub_rn(fabs(__dsub_rn(a, b)), fabs(a)), fabs(b));
            }
        }
        unsigned long long m = __ballot(hit);
        if (!m) continue;
        if (!count) first = idA[base + __ffsll((long long)m) - 1];
        count += __popcll(m);
        while (m) {                                                              // word order = lane order: one running sum
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            sum = __dadd_rn(sum, __shfl(term, l));
        }
    }
}

// return -score / 2.0 (ScoringObject.cpp:57); no common word: -0.0, as on the host
__device__ __forceinline__ double pl_score(double sum) { return __ddiv_rn(-sum, 2.0); }

__global__ __launch_bounds__(256) void k_bow_score_pairs(PgBowTable T, const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                                         int npairs, double* __restrict__ out)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= npairs) return;
    const int a = pa[p], b = pb[p];
    const int nA = pl_len(T, a), nB = pl_len(T, b);
    int count; uint32_t first; double sum;
    pl_overlap(T.id + (int64_t)(nA ? a : 0) * T.cap, T.val + (int64_t)(nA ? a : 0) * T.cap, nA,
               T.id + (int64_t)(nB ? b : 0) * T.cap, T.val + (int64_t)(nB ? b : 0) * T.cap, nB, lane, count, first, sum);
    if (lane == 0) out[p] = pl_score(sum);
}

// BowVector of every frame (TemplatedVocabulary.h:1138-1175 with BowVector::addWeight and ::normalize(L1)): the features with
// weight > 0 sorted by (word id, feature index) -- a stable sort, here by counting ranks on LDS --, each word's weights added in
// feature order from 0.0, the norm as one running sum of fabs in ascending word order, every value divided by it when it is > 0.
__global__ __launch_bounds__(BV_T) void k_bow_vectors(const uint32_t* __restrict__ word, const double* __restrict__ weight,
                                                      const int32_t* __restrict__ nIn, int cap, uint32_t* __restrict__ bowId,
                                                      double* __restrict__ bowVal, int32_t* __restrict__ nbow)
{
    const int f = blockIdx.x, tid = threadIdx.x, n = min(max(nIn[f], 0), cap);
    uint32_t* key = reinterpret_cast<uint32_t*>(pg_sfi_smem);               // [cap] word of feature i
    uint32_t* sword = key + cap;                                              // [cap] sorted words
    uint32_t* sfeat = sword + cap;                                            // [cap] their features
    int* scan = reinterpret_cast<int*>(sfeat + cap);                          // [BV_T + 1]
    uint8_t* ok = reinterpret_cast<uint8_t*>(scan + BV_T + 1);                // [cap] weight > 0
    double* vals = reinterpret_cast<double*>(pg_sfi_smem);                    // [groups] over key / sword, once the ids are out
    __shared__ int sM;
    __shared__ double sNorm;
    word += (int64_t)f * cap; weight += (int64_t)f * cap; bowId += (int64_t)f * cap; bowVal += (int64_t)f * cap;
    if (tid == 0) sM = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += BV_T) {
        const bool v = weight[i] > 0;                                         // not a stopped word (:1157)
        key[i] = word[i]; ok[i] = v; mine += v;
    }
    if (mine) atomicAdd(&sM, mine);
    __syncthreads();
    const int m = sM;
    for (int i = tid; i < n; i += BV_T) {
        if (!ok[i]) continue;
        const uint32_t k = key[i];
        int r = 0;
        for (int j = 0; j < n; j++) { const uint32_t kj = key[j]; r += (ok[j] && (kj < k || (kj == k && j < i))) ? 1 : 0; }
        sword[r] = k; sfeat[r] = (uint32_t)i;
    }
    __syncthreads();
    const int per = (m + BV_T - 1) / BV_T, r0 = tid * per, r1 = min(m, r0 + per);      // per <= 8
    int heads = 0;
    for (int r = r0; r < r1; r++) heads += (r == 0 || sword[r] != sword[r - 1]);
    scan[tid] = heads;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int t = 0; t < BV_T; t++) { const int h = scan[t]; scan[t] = acc; acc += h; } scan[BV_T] = acc; }
    __syncthreads();
    const int nb = scan[BV_T], g0 = scan[tid];
    double sums[BV_MAX / BV_T];
    unsigned headMask = 0u;
#pragma unroll
    for (int k = 0; k < BV_MAX / BV_T; k++) {
        const int r = r0 + k;
        sums[k] = 0.0;
        if (r < r1 && (r == 0 || sword[r] != sword[r - 1])) {
            const uint32_t w = sword[r];
            double v = 0.0;                                                   // v[word] += weight, in feature order (BowVector.cpp:34-46)
            for (int t = r; t < m && sword[t] == w; t++) v = __dadd_rn(v, weight[sfeat[t]]);
            sums[k] = v;
            headMask |= 1u << k;
            bowId[g0 + __popc(headMask) - 1] = w;
        }
    }
    __syncthreads();                                                          // every read of key / sword is done: vals may overlay them
#pragma unroll
    for (int k = 0; k < BV_MAX / BV_T; k++)
        if (headMask & (1u << k)) vals[g0 + __popc(headMask & ((1u << k) - 1u))] = sums[k];
    __syncthreads();
    if (tid == 0) {                                                           // BowVector::normalize(L1) (BowVector.cpp:62-84)
        double norm = 0.0;
        for (int t = 0; t < nb; t++) norm = __dadd_rn(norm, fabs(vals[t]));
        sNorm = norm;
        nbow[f] = nb;
    }
    __syncthreads();
    const double norm = sNorm;
    for (int t = tid; t < nb; t += BV_T) bowVal[t] = norm > 0.0 ? __ddiv_rn(vals[t], norm) : vals[t];
}

struct PgPlaceQuery {
    int nframes, nq, ccap, loop, nconn;
    const uint8_t* inDb; const int32_t* neigh; const int32_t* query; const float* state; const float* minScore;
    const int32_t* connStart; const int32_t* conn;
    // [nq][nframes] rows of the slab: k_place_overlap's results, then k_place_decide's
    int32_t* cnt; uint32_t* first; float* si; float* stored; float* acc; int32_t* bk;
    unsigned long long* slot; unsigned long long* list;
    int32_t* cand; int32_t* ncand; int32_t* common; float* score; int32_t* stats;
};

__global__ __launch_bounds__(256) void k_place_overlap(PgBowTable T, PgPlaceQuery Q)
{
    const int qi = blockIdx.y, kf = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (kf >= Q.nframes) return;
    const int q = Q.query[qi];
    const int nA = pl_len(T, q);
    bool member = nA > 0 && Q.inDb[kf] != 0;                                  // only database members are in an inverted list
    if (member && Q.loop) {                                                   // spConnectedKeyFrames.count(pKFi) (:106-113)
        const int c0 = min(max(Q.connStart[qi], 0), Q.nconn), c1 = min(max(Q.connStart[qi + 1], c0), Q.nconn);
        bool found = false;
        for (int k = c0 + lane; k < c1; k += 64) found |= Q.conn[k] == kf;
        if (__ballot(found)) member = false;
    }
    int count = 0; uint32_t first = 0u; double sum = 0.0;
    if (member) {
        const int nB = pl_len(T, kf);
        pl_overlap(T.id + (int64_t)q * T.cap, T.val + (int64_t)q * T.cap, nA, T.id + (int64_t)kf * T.cap, T.val + (int64_t)kf * T.cap, nB,
                   lane, count, first, sum);
    }
    if (lane == 0) {
        const int64_t o = (int64_t)qi * Q.nframes + kf;
        Q.cnt[o] = count; Q.first[o] = first;
        Q.si[o] = __double2float_rn(pl_score(sum));                          // float si = mpVoc->score(...) (:134, :258)
    }
}

__device__ __forceinline__ unsigned long long pl_load64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(PL_T) void k_place_decide(PgPlaceQuery Q)
{
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nf = Q.nframes;
    const int64_t row = (int64_t)qi * nf;
    const bool loop = Q.loop != 0;
    __shared__ int sMax, sShare, sScored, sN;
    __shared__ float sBest[PL_T / 64];
    if (tid == 0) { sMax = 0; sShare = 0; sScored = 0; sN = 0; }
    __syncthreads();
    int lmax = 0, lshare = 0;
    for (int kf = tid; kf < nf; kf += PL_T) {
        const int c = Q.cnt[row + kf];
        lmax = max(lmax, c); lshare += c > 0;
        if (Q.common) Q.common[row + kf] = c;
    }
    if (lshare) { atomicMax(&sMax, lmax); atomicAdd(&sShare, lshare); }
    __syncthreads();
    const int maxC = sMax;
    const int minC = (int)__fmul_rn((float)maxC, 0.8f);                       // int minCommonWords = maxCommonWords*0.8f (:126, :246)
    int lsc = 0;
    for (int kf = tid; kf < nf; kf += PL_T) {
        const bool scored = Q.cnt[row + kf] > minC;                           // (:133, :253; no sharing key frame: 0 > 0, none)
        const float st = scored ? Q.si[row + kf] : (Q.state ? Q.state[kf] : 0.0f);     // mRelocScore / mLoopScore afterwards
        Q.stored[row + kf] = st;
        if (Q.score) Q.score[row + kf] = st;
        Q.slot[row + kf] = ~0ull;
        lsc += scored;
    }
    if (lsc) atomicAdd(&sScored, lsc);
    __syncthreads();
    const float init = loop ? Q.minScore[qi] : 0.0f;                          // bestAccScore (:159, :273)
    float lm = init;
    for (int kf = tid; kf < nf; kf += PL_T) {
        const float s = Q.si[row + kf];
        bool entry = Q.cnt[row + kf] > minC;
        if (loop && !(s >= init)) entry = false;                              // if(si>=minScore) (:139)
        float a = 0.0f;
        int b = -1;
        if (entry) {
            a = s; b = kf;
            float bs = s;
            for (int j = 0; j < PL_NEIGH; j++) {
                const int nb = Q.neigh[(int64_t)kf * PL_NEIGH + j];
                if ((unsigned)nb >= (unsigned)nf) continue;
                const int cn = Q.cnt[row + nb];
                // mnRelocQuery == id alone (:287): a sharing key frame below the threshold gives its stale score;
                // the loop form also asks mnLoopWords > minCommonWords (:172)
                if (!(loop ? cn > minC : cn > 0)) continue;
                const float v = Q.stored[row + nb];
                a = __fadd_rn(a, v);
                if (v > bs) { b = nb; bs = v; }
            }
            if (a > lm) lm = a;
        }
        Q.acc[row + kf] = a; Q.bk[row + kf] = b;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const float o = __shfl_xor(lm, d); lm = o > lm ? o : lm; }
    if (lane == 0) sBest[wv] = lm;
    __syncthreads();
    float best = sBest[0];
    for (int w = 1; w < PL_T / 64; w++) { const float o = sBest[w]; best = o > best ? o : best; }
    const float keep = __fmul_rn(0.75f, best);                                // minScoreToRetain (:189, :303)
    for (int kf = tid; kf < nf; kf += PL_T) {
        const int b = Q.bk[row + kf];
        if (b >= 0 && Q.acc[row + kf] > keep)                                 // the entry's place in the sharing list names its pBestKF
            atomicMin(&Q.slot[row + b], ((unsigned long long)Q.first[row + kf] << 16) | (unsigned long long)kf);
    }
    __syncthreads();
    for (int b = tid; b < nf; b += PL_T) {
        const unsigned long long k = pl_load64(&Q.slot[row + b]);
        if (k != ~0ull) Q.list[row + atomicAdd(&sN, 1)] = (k << 16) | (unsigned long long)b;
    }
    __syncthreads();
    const int C = sN;
    for (int i = tid; i < C; i += PL_T) {                                     // first occurrence only, in list order: rank by counting
        const unsigned long long me = Q.list[row + i];
        int r = 0;
        for (int j = 0; j < C; j++) r += Q.list[row + j] < me;
        if (r < Q.ccap) Q.cand[(int64_t)qi * Q.ccap + r] = (int)(me & 0xFFFFull);
    }
    if (tid == 0) {
        Q.ncand[qi] = C;
        if (Q.stats) { Q.stats[qi * 3] = sShare; Q.stats[qi * 3 + 1] = maxC; Q.stats[qi * 3 + 2] = sScored; }
    }
}

// the context's vocabulary, when one is uploaded, must score with L1 (the only score these kernels restate)
static int pl_check_scoring(pgorb_ctx* c, bool need_vocab, bool need_tf, const char* who)
{
    int scoring = 0, weighting = 0;
    if (!pg_ctx_vocab_kind(c, &scoring, &weighting)) {
        if (need_vocab) { pg_ctx_fail(c, PGORB_E_ARG, "no vocabulary uploaded"); return PGORB_E_ARG; }
        return 0;
    }
    if (scoring != 0 || (need_tf && weighting != 0 && weighting != 1)) {
        pg_ctx_fail(c, PGORB_E_ARG, who);
        return PGORB_E_ARG;
    }
    return 0;
}

static int pl_launch_queries(pgorb_ctx* c, const PgBowTable& T, PgPlaceQuery Q, hipStream_t s, const char* who)
{
    const size_t rows = (size_t)Q.nq * Q.nframes;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t oCnt = take(rows * 4), oFirst = take(rows * 4), oSi = take(rows * 4), oStored = take(rows * 4), oAcc = take(rows * 4),
                 oBk = take(rows * 4), oSlot = take(rows * 8), oList = take(rows * 8);
    void* scr;
    int rc = pg_ctx_scratch(c, o, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    Q.cnt = (int32_t*)(b + oCnt); Q.first = (uint32_t*)(b + oFirst); Q.si = (float*)(b + oSi); Q.stored = (float*)(b + oStored);
    Q.acc = (float*)(b + oAcc); Q.bk = (int32_t*)(b + oBk); Q.slot = (unsigned long long*)(b + oSlot); Q.list = (unsigned long long*)(b + oList);
    hipLaunchKernelGGL(k_place_overlap, dim3((unsigned)((Q.nframes + 3) / 4), (unsigned)Q.nq), dim3(256), 0, s, T, Q);
    hipLaunchKernelGGL(k_place_decide, dim3((unsigned)Q.nq), dim3(PL_T), 0, s, Q);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, who);
    return pg_ctx_scratch_done(c, s);
}

static int pl_queries(pgorb_ctx* c, bool loop, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nframes, int cap,
                      const uint8_t* d_in_db, const int32_t* d_neigh, const int32_t* d_query, int nq, const float* d_state,
                      const float* d_min_score, const int32_t* d_conn_start, const int32_t* d_conn, int nconn, int32_t* d_cand, int ccap,
                      int32_t* d_ncand, int32_t* d_common, float* d_score, int32_t* d_stats, void* stream)
{
    const char* who = loop ? "bad argument to pgorb_detect_loop_candidates_batch_device" : "bad argument to pgorb_detect_relocalization_candidates_batch_device";
    if (!d_bow_id || !d_bow_val || !d_nbow || nframes < 1 || cap < 1 || !d_in_db || !d_neigh || nq < 0 || ccap < 0 || nconn < 0 ||
        (nq && (!d_query || !d_ncand || (ccap && !d_cand))) || (loop && nq && (!d_min_score || !d_conn_start || (nconn && !d_conn))))
        return pg_ctx_fail(c, PGORB_E_ARG, who);
    if (nframes > PL_MAX_FRAMES) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 65536 frames in the place-recognition table");
    if (nq > 65535) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 65535 queries in one batch");
    if (int rc = pl_check_scoring(c, false, false, "the context's vocabulary does not score with L1_NORM")) return rc;
    if (!nq) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const PgBowTable T = {d_bow_id, d_bow_val, d_nbow, nframes, cap};
    PgPlaceQuery Q = {};
    Q.nframes = nframes; Q.nq = nq; Q.ccap = ccap; Q.loop = loop ? 1 : 0; Q.nconn = nconn;
    Q.inDb = d_in_db; Q.neigh = d_neigh; Q.query = d_query; Q.state = d_state; Q.minScore = d_min_score;
    Q.connStart = d_conn_start; Q.conn = d_conn;
    Q.cand = d_cand; Q.ncand = d_ncand; Q.common = d_common; Q.score = d_score; Q.stats = d_stats;
    return pl_launch_queries(c, T, Q, (hipStream_t)stream, loop ? "k_place_overlap / k_place_decide launch failed (loop)" : "k_place_overlap / k_place_decide launch failed");
}

// one query through host buffers: a one-query batch; the inputs are checked here
static int pl_single(pgorb_ctx* c, bool loop, int nkf, const int32_t* bow_start, const uint32_t* bow_id, const double* bow_val,
                     const uint8_t* in_db, const int32_t* neigh_start, const int32_t* neigh, int query, float* score_state, float min_score,
                     const int32_t* conn, int nconn, int32_t* cand, int ccap, int32_t* common, float* score, int32_t* stats)
{
    const char* fn = loop ? "pgorb_detect_loop_candidates" : "pgorb_detect_relocalization_candidates";
    auto bad = [&](const char* what) { return pg_ctx_fail(c, PGORB_E_ARG, (std::string(fn) + ": " + what).c_str()); };
    if (nkf < 1 || !bow_start || !in_db || !neigh_start || ccap < 0 || (ccap && !cand) || nconn < 0 || (nconn && !conn)) return bad("bad argument");
    if (nkf > PL_MAX_FRAMES) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 65536 frames in the place-recognition table");
    if (int rc = pl_check_scoring(c, false, false, "the context's vocabulary does not score with L1_NORM")) return rc;
    if (query < 0 || query >= nkf) return bad("the query index is out of range");
    if (bow_start[0] != 0 || neigh_start[0] != 0) return bad("a start array does not begin at 0");
    int cap = 1;
    for (int f = 0; f < nkf; f++) {
        if (bow_start[f + 1] < bow_start[f] || neigh_start[f + 1] < neigh_start[f]) return bad("a start array decreases");
        if (neigh_start[f + 1] - neigh_start[f] > PL_NEIGH) return bad("a neighbour list is longer than 10");
        cap = std::max(cap, bow_start[f + 1] - bow_start[f]);
    }
    const int nwords = bow_start[nkf], nneigh = neigh_start[nkf];
    if ((nwords && (!bow_id || !bow_val)) || (nneigh && !neigh)) return bad("bad argument");
    for (int f = 0; f < nkf; f++)
        for (int k = bow_start[f] + 1; k < bow_start[f + 1]; k++)
            if (!(bow_id[k - 1] < bow_id[k])) return bad("a BowVector's word ids are unsorted or repeat");
    for (int k = 0; k < nneigh; k++) if (neigh[k] < 0 || neigh[k] >= nkf) return bad("a neighbour index is out of range");
    for (int k = 0; k < nconn; k++) if (conn[k] < 0 || conn[k] >= nkf) return bad("a connected key frame index is out of range");
    if ((size_t)nkf * cap > ((size_t)1 << 28)) return pg_ctx_fail(c, PGORB_E_LIMIT, "the padded BowVector table exceeds 2^28 entries");

    PgHostCall hc(c);
    const size_t tab = (size_t)nkf * cap;
    const size_t oId = hc.region(PG_UP, tab * 4), oVal = hc.region(PG_UP, tab * 8), oN = hc.region(PG_UP, (size_t)nkf * 4), oDb = hc.region(PG_UP, nkf),
                 oNe = hc.region(PG_UP, (size_t)nkf * PL_NEIGH * 4), oQ = hc.region(PG_UP, 4), oSt = hc.region(PG_UP, (size_t)nkf * 4),
                 oMin = hc.region(PG_UP, 4), oCs = hc.region(PG_UP, 8), oCo = hc.region(PG_UP, (size_t)std::max(nconn, 1) * 4),
                 oCand = hc.region(PG_DOWN, (size_t)std::max(ccap, 1) * 4), oNc = hc.region(PG_DOWN, 4), oCom = hc.region(PG_DOWN, (size_t)nkf * 4),
                 oSc = hc.region(PG_DOWN, (size_t)nkf * 4), oStats = hc.region(PG_DOWN, 12);
    int rc = hc.begin();
    if (rc) return rc;
    hc.put(oId, nullptr, 0, 0, tab * 4);
    hc.put(oVal, nullptr, 0, 0, tab * 8);
    int32_t* hn = hc.host<int32_t>(oN);
    int32_t* hne = hc.host<int32_t>(oNe);
    for (int f = 0; f < nkf; f++) {
        const int nb = bow_start[f + 1] - bow_start[f], nn = neigh_start[f + 1] - neigh_start[f];
        hn[f] = nb;
        if (nb) { hc.put(oId, bow_id + bow_start[f], (size_t)nb * 4, (size_t)f * cap * 4); hc.put(oVal, bow_val + bow_start[f], (size_t)nb * 8, (size_t)f * cap * 8); }
        for (int j = 0; j < PL_NEIGH; j++) hne[f * PL_NEIGH + j] = j < nn ? neigh[neigh_start[f] + j] : -1;
    }
    hc.put(oDb, in_db, nkf);
    hc.put(oQ, &query, 4);
    hc.put(oSt, score_state, (size_t)nkf * 4, 0, (size_t)nkf * 4);            // NULL: 0.0f
    hc.put(oMin, &min_score, 4);
    const int32_t cs[2] = {0, nconn};
    hc.put(oCs, cs, 8);
    hc.put(oCo, conn, (size_t)nconn * 4);
    if ((rc = hc.run([&] {
            return pl_queries(c, loop, hc.dev<uint32_t>(oId), hc.dev<double>(oVal), hc.dev<int32_t>(oN), nkf, cap, hc.dev(oDb), hc.dev<int32_t>(oNe),
                              hc.dev<int32_t>(oQ), 1, loop ? nullptr : hc.dev<float>(oSt), hc.dev<float>(oMin), hc.dev<int32_t>(oCs), hc.dev<int32_t>(oCo),
                              nconn, hc.dev<int32_t>(oCand), ccap, hc.dev<int32_t>(oNc), hc.dev<int32_t>(oCom), hc.dev<float>(oSc),
                              hc.dev<int32_t>(oStats), nullptr); }))) return rc;
    const int nc = *hc.host<int32_t>(oNc);
    if (cand) memcpy(cand, hc.host(oCand), (size_t)std::min(nc, ccap) * 4);
    if (common) memcpy(common, hc.host(oCom), (size_t)nkf * 4);
    if (score_state && !loop) memcpy(score_state, hc.host(oSc), (size_t)nkf * 4);
    if (score) memcpy(score, hc.host(oSc), (size_t)nkf * 4);
    if (stats) memcpy(stats, hc.host(oStats), 12);
    return nc;
}

extern "C" {

int pgorb_bow_vectors_batch_device(pgorb_ctx* c, const uint32_t* d_word, const double* d_weight, const int32_t* d_n, int nframes, int cap,
                                   uint32_t* d_bow_id, double* d_bow_val, int32_t* d_nbow, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_word || !d_weight || !d_n || nframes < 1 || cap < 1 || !d_bow_id || !d_bow_val || !d_nbow)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_bow_vectors_batch_device");
    if (int rc = pl_check_scoring(c, true, true, "pgorb_bow_vectors_batch_device: the vocabulary is not L1_NORM with TF_IDF or TF")) return rc;
    if (cap > BV_MAX) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 8192 features per frame");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const size_t lds = (size_t)cap * 13 + (BV_T + 1) * 4 + 16;
    if (!pg_raise_lds<k_bow_vectors>(c, lds)) return pg_ctx_fail(c, PGORB_E_LIMIT, "BowVector scratch exceeds the LDS");
    hipLaunchKernelGGL(k_bow_vectors, dim3((unsigned)nframes), dim3(BV_T), lds, (hipStream_t)stream, d_word, d_weight, d_n, cap, d_bow_id, d_bow_val, d_nbow);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_bow_vectors launch failed");
    return 0;
}

int pgorb_bow_score_l1_batch_device(pgorb_ctx* c, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nframes, int cap,
                                    const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, double* d_score, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_bow_id || !d_bow_val || !d_nbow || nframes < 1 || cap < 1 || npairs < 0 || (npairs && (!d_pair_a || !d_pair_b || !d_score)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_bow_score_l1_batch_device");
    if (int rc = pl_check_scoring(c, false, false, "the context's vocabulary does not score with L1_NORM")) return rc;
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const PgBowTable T = {d_bow_id, d_bow_val, d_nbow, nframes, cap};
    hipLaunchKernelGGL(k_bow_score_pairs, dim3((unsigned)((npairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, T, d_pair_a, d_pair_b, npairs, d_score);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_bow_score_pairs launch failed");
    return 0;
}

int pgorb_detect_relocalization_candidates_batch_device(pgorb_ctx* c, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow,
                                                        int nframes, int cap, const uint8_t* d_in_db, const int32_t* d_neigh,
                                                        const int32_t* d_query, int nq, const float* d_score_state, int32_t* d_cand, int ccap,
                                                        int32_t* d_ncand, int32_t* d_common, float* d_score, int32_t* d_stats, void* stream)
{
    if (!c) return PGORB_E_ARG;
    return pl_queries(c, false, d_bow_id, d_bow_val, d_nbow, nframes, cap, d_in_db, d_neigh, d_query, nq, d_score_state, nullptr, nullptr, nullptr, 0,
                      d_cand, ccap, d_ncand, d_common, d_score, d_stats, stream);
}

int pgorb_detect_loop_candidates_batch_device(pgorb_ctx* c, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nframes,
                                              int cap, const uint8_t* d_in_db, const int32_t* d_neigh, const int32_t* d_query, int nq,
                                              const float* d_min_score, const int32_t* d_conn_start, const int32_t* d_conn, int nconn,
                                              int32_t* d_cand, int ccap, int32_t* d_ncand, int32_t* d_common, float* d_score, int32_t* d_stats,
                                              void* stream)
{
    if (!c) return PGORB_E_ARG;
    return pl_queries(c, true, d_bow_id, d_bow_val, d_nbow, nframes, cap, d_in_db, d_neigh, d_query, nq, nullptr, d_min_score, d_conn_start, d_conn,
                      nconn, d_cand, ccap, d_ncand, d_common, d_score, d_stats, stream);
}

int pgorb_detect_relocalization_candidates(pgorb_ctx* c, int nkf, const int32_t* bow_start, const uint32_t* bow_id, const double* bow_val,
                                           const uint8_t* in_db, const int32_t* neigh_start, const int32_t* neigh, int query, float* score_state,
                                           int32_t* cand, int ccap, int32_t* common, int32_t* stats)
{
    if (!c) return PGORB_E_ARG;
    return pl_single(c, false, nkf, bow_start, bow_id, bow_val, in_db, neigh_start, neigh, query, score_state, 0.0f, nullptr, 0, cand, ccap, common,
                     nullptr, stats);
}

int pgorb_detect_loop_candidates(pgorb_ctx* c, int nkf, const int32_t* bow_start, const uint32_t* bow_id, const double* bow_val,
                                 const uint8_t* in_db, const int32_t* neigh_start, const int32_t* neigh, int query, float min_score,
                                 const int32_t* conn, int nconn, int32_t* cand, int ccap, int32_t* common, float* score, int32_t* stats)
{
    if (!c) return PGORB_E_ARG;
    return pl_single(c, true, nkf, bow_start, bow_id, bow_val, in_db, neigh_start, neigh, query, nullptr, min_score, conn, nconn, cand, ccap, common,
                     score, stats);
}

}  // extern "C"
