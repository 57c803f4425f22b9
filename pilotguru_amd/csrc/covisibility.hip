// covisibility.hip -- the covisibility graph next to the map-point table, on gfx950: KeyFrame::UpdateConnections of a list of key
// frames, the views the other entry points read, and Tracking::UpdateLocalMap of many frames.  Integers only.
//
// Restates (thirdparty/orb-slam2):
//   KeyFrame::UpdateConnections                 src/KeyFrame.cc:392-482
//   KeyFrame::AddConnection / UpdateBestCovisibles   src/KeyFrame.cc:226-260
//   GetBestCovisibilityKeyFrames / GetCovisiblesByWeight   src/KeyFrame.cc:277-302
//   LoopConnections of LoopClosing::CorrectLoop src/LoopClosing.cc:548-566
//   Tracking::UpdateLocalKeyFrames / UpdateLocalPoints   src/Tracking.cc:1196-1321
//
// UpdateConnections of the list, one key frame after another, decomposes exactly: the counters c_i depend on
// the map alone, so every list member's update is known without running the ones before it, and a row ends as its base (its own
// update, or its input) overwritten by the AddConnection calls of the members that come later in the list.
//   k_cov_prep     the position of each key frame in the list and the inverse of kf_order (address rank -> key frame)
//   k_cov_count    a workgroup per list member: slots -> points -> observation lists -> LDS counters per key frame; the dense
//                  counter row, the number of keys and the fallback target (pKFmax) go to the scratch arena
//   k_cov_finish   a workgroup per key frame: the row's map as a dense LDS array, the sends before and after its own update, the
//                  two sorts (address order; descending (weight, address)) as one bitonic sort of 64-bit keys in LDS
//   k_cov_loop     LoopConnections in map-then-set address order, padded with (-1, -1, 0)
//   k_cov_views    GetBestCovisibilityKeyFrames(nbest), the essential graph's CSR, the length of GetCovisiblesByWeight(w)
//   k_cov_local    a workgroup per frame: votes by LDS atomics, the first stage by a scan in address order, the short sequential
//                  expansion, and the point union ordered by a first-position key per table point and a scan
#include "match_common.h"
#include <string>

#define COV_T 256
#define COV_ABSENT INT32_MIN

struct PgCovBatch {
    const int32_t* kfPoint; const int32_t* n; int nframes; int cap;
    int npoints; const uint8_t* pbad; const int32_t* obsStart; const int32_t* obsFrame; int nobs;
    const int32_t* order; const uint8_t* id0;
    int nlist; const int32_t* list; int th;
    int connCap; int32_t* connKf; int32_t* connW; int32_t* nconn; int32_t* ordKf; int32_t* ordW; int32_t* nord;
    int32_t* parent; uint8_t* first; int32_t* rowStatus; int loopCap; int32_t* loopConn; int32_t* info;
    // scratch
    int32_t* pos; int32_t* inv; int32_t* meta; int32_t* lcCount; int32_t* W; uint8_t* lcFlag;
};

// the address rank of key frame f, or -1 when kf_order gives it none of its own
__device__ __forceinline__ int cov_rank(const int32_t* order, const int32_t* inv, int nframes, int f)
{
    if (!order) return f;
    const int r = order[f];
    return (r >= 0 && r < nframes && inv[r] == f) ? r : -1;
}

// exclusive position of a set flag among the workgroup's COV_T threads, and the total; every thread calls it
__device__ __forceinline__ int cov_scan(bool flag, int* sWave, int& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();
    if (lane == 0) sWave[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < COV_T / 64; k++) { if (k < w) base += sWave[k]; total += sWave[k]; }
    return base + __popcll(m & ((1ull << lane) - 1));
}

// ascending bitonic sort of key[0 .. m), m a power of two, by the whole workgroup
__device__ __forceinline__ void cov_sort(unsigned long long* key, int m)
{
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < m; t += COV_T) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long a = key[t], b = key[x];
                    if (((t & k) == 0) ? (a > b) : (a < b)) { key[t] = b; key[x] = a; }
                }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(COV_T) void k_cov_prep(const int32_t* __restrict__ order, int nframes, const int32_t* __restrict__ list, int nlist,
                                                     int32_t* __restrict__ inv, int32_t* __restrict__ pos)
{
    const int t = blockIdx.x * COV_T + threadIdx.x;
    if (t < nframes) {
        const int r = order ? order[t] : t;
        if (r >= 0 && r < nframes) atomicMax(&inv[r], t);              // a rank named twice belongs to the larger index, whatever runs first
    }
    if (pos && t < nlist) {
        const int f = list[t];
        if (f >= 0 && f < nframes) atomicMax(&pos[f], t);
    }
}

__global__ __launch_bounds__(COV_T) void k_cov_count(PgCovBatch B)
{
    __shared__ int32_t sCnt[PGORB_COVIS_MAX_KF];
    __shared__ unsigned long long sMax;
    __shared__ int sKeys, sSends;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int i = B.list[k];
    int32_t* meta = B.meta + 4 * (int64_t)k;
    if (i < 0 || i >= B.nframes || B.pos[i] != k || cov_rank(B.order, B.inv, B.nframes, i) < 0) {   // no key frame, or named again later in the list
        if (tid == 0) { meta[0] = 0; meta[1] = 0; meta[2] = -2; meta[3] = 0; }
        return;
    }
    for (int f = tid; f < B.nframes; f += COV_T) sCnt[f] = 0;
    if (tid == 0) { sMax = 0; sKeys = 0; sSends = 0; }
    __syncthreads();
    const int n = min(max(B.n[i], 0), B.cap);
    for (int s = tid; s < n; s += COV_T) {                                 // :405-423
        const int p = B.kfPoint[(int64_t)i * B.cap + s];
        if (p < 0 || p >= B.npoints || (B.pbad && B.pbad[p])) continue;
        const int a = B.obsStart[p], b = B.obsStart[p + 1];
        if (a < 0 || b < a || b > B.nobs) continue;
        for (int o = a; o < b; o++) {
            const int f = B.obsFrame[o];
            if (f < 0 || f >= B.nframes || f == i) continue;               // mit->first->mnId==mnId
            atomicAdd(&sCnt[f], 1);
        }
    }
    __syncthreads();
    int keys = 0, sends = 0;
    unsigned long long best = 0;
    for (int f = tid; f < B.nframes; f += COV_T) {
        int c = sCnt[f];
        const int r = c > 0 ? cov_rank(B.order, B.inv, B.nframes, f) : -1;
        if (r < 0) c = 0;
        B.W[(int64_t)k * B.nframes + f] = c;
        if (c > 0) {
            keys++;
            sends += c >= B.th;
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7FFFFFFF - r);   // the first strict maximum (:439-443)
            best = max(best, key);
        }
    }
    if (keys) { atomicAdd(&sKeys, keys); atomicAdd(&sSends, sends); atomicMax(&sMax, best); }
    __syncthreads();
    if (tid == 0) {
        meta[0] = sKeys; meta[1] = sSends;
        meta[2] = !sKeys ? -2 : sSends ? -1 : B.inv[0x7FFFFFFF - (int)(unsigned)(sMax & 0xFFFFFFFFu)];
        meta[3] = 0;
    }
}

// what list member kk sends to key frame i (AddConnection(this, weight), :447 and :454), 0 for nothing
__device__ __forceinline__ int cov_send(const PgCovBatch& B, int kk, int i)
{
    const int32_t* m = B.meta + 4 * (int64_t)kk;
    const int fb = m[2];
    if (fb == -2) return 0;
    const int c = B.W[(int64_t)kk * B.nframes + i];
    return (fb == -1 ? c >= B.th : fb == i) ? c : 0;
}

__global__ __launch_bounds__(COV_T) void k_cov_finish(PgCovBatch B)
{
    __shared__ int32_t sM[PGORB_COVIS_MAX_KF];
    __shared__ uint8_t sP[PGORB_COVIS_MAX_KF];
    __shared__ unsigned long long sKey[PGORB_COVIS_MAX_CONN];
    __shared__ int sChB, sCh, sN;
    __shared__ unsigned long long sFront;
    const int i = blockIdx.x, tid = threadIdx.x, nf = B.nframes;
    const int pi = B.pos[i];
    const bool member = pi >= 0;
    const int32_t* mine = B.meta + 4 * (int64_t)max(pi, 0);              // read for a list member only
    const bool own = member && mine[0] > 0;
    const int fb = member ? mine[2] : -2;
    const int64_t row = (int64_t)i * B.connCap;
    const int ncIn = min(max(B.nconn[i], 0), B.connCap), noIn = min(max(B.nord[i], 0), B.connCap);
    for (int f = tid; f < nf; f += COV_T) { sM[f] = COV_ABSENT; sP[f] = 0; }
    if (tid == 0) { sChB = 0; sCh = 0; sN = 0; sFront = 0; }
    __syncthreads();
    for (int t = tid; t < ncIn; t += COV_T) {                              // the input map
        const int f = B.connKf[row + t];
        if (f >= 0 && f < nf && f != i && cov_rank(B.order, B.inv, nf, f) >= 0) sM[f] = B.connW[row + t];
    }
    __syncthreads();
    for (int kk = tid; kk < pi; kk += COV_T) {                             // AddConnection by the members before this one
        const int c = cov_send(B, kk, i);
        if (c > 0) { const int j = B.list[kk]; if (sM[j] != c) sChB = 1; sM[j] = c; }
    }
    __syncthreads();
    const bool chB = sChB != 0;
    if (member) {                                                          // GetVectorCovisibleKeyFrames() just before the own update (LoopClosing.cc:553)
        if (chB) { for (int f = tid; f < nf; f += COV_T) sP[f] = sM[f] != COV_ABSENT; }
        else for (int t = tid; t < noIn; t += COV_T) { const int f = B.ordKf[row + t]; if (f >= 0 && f < nf) sP[f] = 1; }
    }
    __syncthreads();
    if (own) {                                                             // = KFcounter (:470); front() of the own list is the parent (:476)
        const int fbo = fb;
        for (int f = tid; f < nf; f += COV_T) {
            const int c = B.W[(int64_t)pi * nf + f];
            sM[f] = c > 0 ? c : COV_ABSENT;
            if (c > 0 && (fbo == -1 ? c >= B.th : fbo == f))
                atomicMax(&sFront, ((unsigned long long)(unsigned)c << 32) | (unsigned)cov_rank(B.order, B.inv, nf, f));
        }
    } else if (tid == 0) sCh = chB;
    __syncthreads();
    for (int kk = (member ? pi + 1 : 0) + tid; kk < B.nlist; kk += COV_T) {   // AddConnection by the members after it
        const int c = cov_send(B, kk, i);
        if (c > 0) { const int j = B.list[kk]; if (sM[j] != c) sCh = 1; sM[j] = c; }
    }
    __syncthreads();
    const bool changed = sCh != 0;
    int cnt = 0;
    for (int f = tid; f < nf; f += COV_T) cnt += sM[f] != COV_ABSENT;
    if (cnt) atomicAdd(&sN, cnt);
    __syncthreads();
    const int nc = sN;
    __syncthreads();                                                       // every thread has read sN before it is reset below
    if (nc > B.connCap) {                                                  // the row keeps its input bytes
        if (tid == 0) { B.rowStatus[i] = PGORB_COVIS_LIMIT; if (member) B.lcCount[pi] = 0; }
        return;
    }
    const bool touched = own || changed;
    if (!touched && !member) { if (tid == 0) B.rowStatus[i] = 0; return; }
    // mConnectedKeyFrameWeights in address order
    int m2 = 1;
    while (m2 < nc) m2 <<= 1;
    for (int t = tid; t < m2; t += COV_T) sKey[t] = ~0ull;
    if (tid == 0) sN = 0;
    __syncthreads();
    for (int f = tid; f < nf; f += COV_T)
        if (sM[f] != COV_ABSENT) sKey[atomicAdd(&sN, 1)] = (unsigned long long)(unsigned)cov_rank(B.order, B.inv, nf, f);
    cov_sort(sKey, m2);
    int lc = 0;
    for (int t = tid; t < nc; t += COV_T) {
        const int f = B.inv[(int)sKey[t]];
        if (touched) { B.connKf[row + t] = f; B.connW[row + t] = sM[f]; }
        if (member) {                                                      // LoopConnections[pKFi] (LoopClosing.cc:557-565)
            const bool l = !sP[f] && B.pos[f] < 0;
            B.lcFlag[(int64_t)pi * B.connCap + t] = l;
            lc += l;
        }
    }
    __syncthreads();
    if (tid == 0) sN = 0;
    __syncthreads();
    if (lc) atomicAdd(&sN, lc);
    __syncthreads();
    if (member && tid == 0) B.lcCount[pi] = sN;
    int status = own ? PGORB_COVIS_UPDATED | (fb >= 0 ? PGORB_COVIS_FALLBACK : 0) : member ? PGORB_COVIS_EMPTY : 0;
    if (changed) status |= PGORB_COVIS_RESORTED;
    if (touched) {
        // the ordered list: descending (weight, address) of the whole map after a changed AddConnection (:241-260), else of the own sends
        __syncthreads();
        for (int t = tid; t < m2; t += COV_T) sKey[t] = ~0ull;
        if (tid == 0) sN = 0;
        __syncthreads();
        for (int f = tid; f < nf; f += COV_T) {
            const int c = sM[f];
            if (c == COV_ABSENT) continue;
            if (!changed && !(fb == -1 ? c >= B.th : fb == f)) continue;
            const unsigned long long key = ((unsigned long long)((unsigned)c ^ 0x80000000u) << 32) | (unsigned)cov_rank(B.order, B.inv, nf, f);
            sKey[atomicAdd(&sN, 1)] = ~key;
        }
        cov_sort(sKey, m2);
        const int no = sN;
        for (int t = tid; t < no; t += COV_T) {
            const unsigned long long key = ~sKey[t];
            B.ordKf[row + t] = B.inv[(int)(unsigned)(key & 0xFFFFFFFFu)];
            B.ordW[row + t] = (int)((unsigned)(key >> 32) ^ 0x80000000u);
        }
        if (tid == 0) {
            B.nconn[i] = nc; B.nord[i] = no;
            if (own && B.first[i] && !(B.id0 && B.id0[i])) {               // :474-479
                B.parent[i] = B.inv[(int)(unsigned)(sFront & 0xFFFFFFFFu)];
                B.first[i] = 0;
                status |= PGORB_COVIS_PARENT_SET;
            }
        }
    }
    if (tid == 0) B.rowStatus[i] = status;
}

__global__ __launch_bounds__(COV_T) void k_cov_loop(PgCovBatch B)
{
    __shared__ int sWave[COV_T / 64];
    __shared__ int sOff, sTotal, sLim;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int i = k < B.nlist ? B.list[k] : -1;
    const bool live = i >= 0 && i < B.nframes && B.pos[i] == k;
    const int myRank = live ? cov_rank(B.order, B.inv, B.nframes, i) : -1;
    if (tid == 0) { sOff = 0; sTotal = 0; sLim = 0; }
    __syncthreads();
    int off = 0, tot = 0;
    for (int kk = tid; kk < B.nlist; kk += COV_T) {
        const int j = B.list[kk];
        if (j < 0 || j >= B.nframes || B.pos[j] != kk) continue;
        const int r = cov_rank(B.order, B.inv, B.nframes, j);
        if (r < 0) continue;
        const int c = B.lcCount[kk];
        tot += c;
        if (r < myRank) off += c;
    }
    if (tot) atomicAdd(&sTotal, tot);
    if (off) atomicAdd(&sOff, off);
    if (k == 0) { int lim = 0; for (int f = tid; f < B.nframes; f += COV_T) lim += B.rowStatus[f] == PGORB_COVIS_LIMIT; if (lim) atomicAdd(&sLim, lim); }
    __syncthreads();
    const int total = sTotal;
    const bool over = B.loopConn && total > B.loopCap;                      // no records asked for: nothing can overflow
    if (k == 0 && tid == 0) { B.info[0] = over ? PGORB_COVIS_LIMIT : 0; B.info[1] = total; B.info[2] = sLim; B.info[3] = 0; }
    if (!B.loopConn) return;
    for (int e = (over ? 0 : total) + k * COV_T + tid; e < B.loopCap; e += gridDim.x * COV_T) {   // no candidate to the essential graph
        B.loopConn[3 * (int64_t)e] = -1; B.loopConn[3 * (int64_t)e + 1] = -1; B.loopConn[3 * (int64_t)e + 2] = 0;
    }
    if (over || !live || myRank < 0 || B.lcCount[k] == 0) return;
    const int nc = min(max(B.nconn[i], 0), B.connCap);
    int base = sOff;
    for (int t0 = 0; t0 < nc; t0 += COV_T) {
        const int t = t0 + tid;
        const bool l = t < nc && B.lcFlag[(int64_t)k * B.connCap + t];
        int chunk;
        const int at = base + cov_scan(l, sWave, chunk);
        if (l) {
            B.loopConn[3 * (int64_t)at] = i;
            B.loopConn[3 * (int64_t)at + 1] = B.connKf[(int64_t)i * B.connCap + t];
            B.loopConn[3 * (int64_t)at + 2] = B.connW[(int64_t)i * B.connCap + t];   // GetWeight (Optimizer.cc:866)
        }
        base += chunk;
    }
}

__global__ __launch_bounds__(64) void k_cov_views(int nframes, int connCap, const int32_t* __restrict__ ordKf, const int32_t* __restrict__ ordW,
                                                   const int32_t* __restrict__ nord, int nbest, int32_t* __restrict__ best, int ncovisCap,
                                                   int32_t* __restrict__ covisStart, int32_t* __restrict__ covis, int32_t* __restrict__ covisW, int w,
                                                   int32_t* __restrict__ byWeight, int32_t* __restrict__ info)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(nord[i], 0), connCap);
    const int64_t row = (int64_t)i * connCap;
    if (best) for (int t = lane; t < nbest; t += 64) best[(int64_t)i * nbest + t] = t < n ? ordKf[row + t] : -1;   // KeyFrame.cc:277-285
    if (byWeight) {                                                        // upper_bound(.., w, weightComp): the first weight below w; none -> EMPTY (:294-296)
        int len = 0;
        for (int t = lane; t < n; t += 64) len += ordW[row + t] >= w;
        for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o);
        if (lane == 0) byWeight[i] = len == n ? 0 : len;
    }
    if (!covisStart) { if (i == 0 && lane == 0) { info[0] = 0; info[1] = 0; } return; }
    int before = 0, total = 0;
    for (int f = lane; f < nframes; f += 64) {
        const int c = min(max(nord[f], 0), connCap);
        total += c;
        if (f < i) before += c;
    }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); total += __shfl_xor(total, o); }
    const bool over = total > ncovisCap;
    if (lane == 0) {
        covisStart[i] = over ? 0 : before;
        if (i == 0) { covisStart[nframes] = over ? 0 : total; info[0] = over ? PGORB_COVIS_LIMIT : 0; info[1] = total; }
    }
    if (over) return;
    for (int t = lane; t < n; t += 64) { covis[before + t] = ordKf[row + t]; covisW[before + t] = ordW[row + t]; }
}

struct PgLocalMapBatch {
    const int32_t* kfPoint; const int32_t* n; int nframes; int cap; const uint8_t* kfBad;
    const int32_t* pairFrame; int npairs; const int32_t* kpPoint;
    int npoints; const uint8_t* pbad; const int32_t* obsStart; const int32_t* obsFrame; int nobs;
    int connCap; const int32_t* ordKf; const int32_t* nord; const int32_t* parent; const int32_t* order;
    int nbest; int maxLocal; int lkfCap; const int32_t* prevKf; const int32_t* nprev;
    int32_t* kpOut; int32_t* localKf; int32_t* nlocal; int32_t* refKf; int qcap; int32_t* queries; int32_t* nq; int32_t* status;
    const int32_t* inv; unsigned* firstKey;
};

__global__ __launch_bounds__(COV_T) void k_cov_local(PgLocalMapBatch B)
{
    __shared__ int32_t sVote[PGORB_COVIS_MAX_KF];
    __shared__ int32_t sList[PGORB_COVIS_MAX_KF];
    __shared__ uint8_t sMark[PGORB_COVIS_MAX_KF];
    __shared__ int sWave[COV_T / 64];
    __shared__ unsigned long long sMax;
    __shared__ int sAny, sSize, sStop, sOver;
    __shared__ unsigned sChild;
    const int p = blockIdx.x, tid = threadIdx.x, nf = B.nframes;
    int fr = B.pairFrame ? B.pairFrame[p] : p;
    const int n = (fr >= 0 && fr < nf) ? min(max(B.n[fr], 0), B.cap) : 0;
    for (int f = tid; f < nf; f += COV_T) { sVote[f] = 0; sMark[f] = 0; }
    if (tid == 0) { sMax = 0; sAny = 0; sSize = 0; sStop = 0; sOver = 0; }
    __syncthreads();
    for (int s = tid; s < n; s += COV_T) {                                 // Tracking.cc:1217-1233
        int q = B.kpPoint[(int64_t)p * B.cap + s];
        if (q >= 0 && q < B.npoints) {
            if (B.pbad && B.pbad[q]) q = -1;                               // mCurrentFrame.mvpMapPoints[i]=NULL
            else {
                const int a = B.obsStart[q], b = B.obsStart[q + 1];
                if (a >= 0 && b >= a && b <= B.nobs)
                    for (int o = a; o < b; o++) {
                        const int f = B.obsFrame[o];
                        if (f >= 0 && f < nf && cov_rank(B.order, B.inv, nf, f) >= 0) { atomicAdd(&sVote[f], 1); sAny = 1; }
                    }
            }
        }
        if (B.kpOut) B.kpOut[(int64_t)p * B.cap + s] = q;
    }
    __syncthreads();
    int status = 0, ref = -1;
    if (!sAny) {                                                           // :1235-1236: the previous list is walked again
        status = PGORB_LOCALMAP_NO_VOTES;
        const int np = B.prevKf ? min(max(B.nprev[p], 0), B.lkfCap) : 0;
        for (int t = tid; t < np; t += COV_T) sList[t] = B.prevKf[(int64_t)p * B.lkfCap + t];
        if (tid == 0) sSize = np;
        __syncthreads();
    } else {
        int size = 0;
        for (int r0 = 0; r0 < nf; r0 += COV_T) {                           // :1245-1260, in address order
            const int r = r0 + tid;
            const int f = r < nf ? B.inv[r] : -1;
            const bool in = f >= 0 && sVote[f] > 0 && !(B.kfBad && B.kfBad[f]);
            int chunk;
            const int at = size + cov_scan(in, sWave, chunk);
            if (in) {
                if (at < B.lkfCap) sList[at] = f;
                sMark[f] = 1;
                atomicMax(&sMax, ((unsigned long long)(unsigned)sVote[f] << 32) | (unsigned)(0x7FFFFFFF - r));
            }
            size += chunk;
        }
        __syncthreads();
        if (sMax) ref = B.inv[0x7FFFFFFF - (int)(unsigned)(sMax & 0xFFFFFFFFu)];
        const int n1 = size;
        if (tid == 0) { sSize = size; sOver = size > B.lkfCap; }
        __syncthreads();
        for (int e = 0; e < n1 && !sOver; e++) {                           // :1264-1314, over the first-stage entries only
            if (sSize > B.maxLocal || sStop) break;
            const int i = sList[e];
            __syncthreads();
            if (tid == 0) {
                sChild = 0xFFFFFFFFu;
                const int nb = min(min(max(B.nord[i], 0), B.connCap), B.nbest);
                for (int t = 0; t < nb; t++) {                             // GetBestCovisibilityKeyFrames(10)
                    const int c = B.ordKf[(int64_t)i * B.connCap + t];
                    if (c < 0 || c >= nf || (B.kfBad && B.kfBad[c]) || sMark[c]) continue;
                    if (sSize < B.lkfCap) sList[sSize] = c; else sOver = 1;
                    sSize++; sMark[c] = 1;
                    break;
                }
            }
            __syncthreads();
            for (int r = tid; r < nf; r += COV_T) {                        // GetChilds(): a std::set<KeyFrame*>
                const int c = B.inv[r];
                if (c >= 0 && B.parent[c] == i && !(B.kfBad && B.kfBad[c]) && !sMark[c]) { atomicMin(&sChild, (unsigned)r); break; }
            }
            __syncthreads();
            if (tid == 0) {
                if (sChild != 0xFFFFFFFFu) {
                    const int c = B.inv[sChild];
                    if (sSize < B.lkfCap) sList[sSize] = c; else sOver = 1;
                    sSize++; sMark[c] = 1;
                }
                const int pp = B.parent[i];                                // no isBad() test, and the break leaves the outer loop
                if (pp >= 0 && pp < nf && !sMark[pp]) {
                    if (sSize < B.lkfCap) sList[sSize] = pp; else sOver = 1;
                    sSize++; sMark[pp] = 1;
                    sStop = 1;
                }
            }
            __syncthreads();
        }
        __syncthreads();
    }
    const bool overKf = sOver != 0;
    const int nl = overKf ? 0 : sSize;
    // UpdateLocalPoints (:1196-1210): the first place of each point in (list order, slot order)
    unsigned* first = B.firstKey + (int64_t)p * B.npoints;
    for (int e = 0; e < nl; e++) {
        const int f = sList[e];
        if (f < 0 || f >= nf) continue;
        const int m = min(max(B.n[f], 0), B.cap);
        for (int s = tid; s < m; s += COV_T) {
            const int q = B.kfPoint[(int64_t)f * B.cap + s];
            if (q >= 0 && q < B.npoints && !(B.pbad && B.pbad[q])) atomicMin(&first[q], (unsigned)e * (unsigned)B.cap + (unsigned)s);
        }
    }
    __threadfence_block();
    __syncthreads();
    int nq = 0;
    for (int e = 0; e < nl; e++) {
        const int f = sList[e];
        if (f < 0 || f >= nf) continue;
        const int m = min(max(B.n[f], 0), B.cap);
        for (int s0 = 0; s0 < m; s0 += COV_T) {
            const int s = s0 + tid;
            const int q = s < m ? B.kfPoint[(int64_t)f * B.cap + s] : -1;
            const bool in = q >= 0 && q < B.npoints && !(B.pbad && B.pbad[q]) &&
                            __hip_atomic_load(&first[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)e * (unsigned)B.cap + (unsigned)s;
            int chunk;
            const int at = nq + cov_scan(in, sWave, chunk);
            if (in && at < B.qcap) B.queries[(int64_t)p * B.qcap + at] = q;
            nq += chunk;
        }
    }
    const bool over = overKf || nq > B.qcap;
    if (over) status |= PGORB_LOCALMAP_LIMIT;
    for (int t = tid; t < nl && !over; t += COV_T) B.localKf[(int64_t)p * B.lkfCap + t] = sList[t];
    if (tid == 0) {
        B.nlocal[p] = over ? 0 : nl;
        B.nq[p] = over ? 0 : nq;
        B.refKf[p] = ref;
        B.status[p] = status;
    }
}

extern "C" {

int pgorb_update_connections_batch_device(pgorb_ctx* c, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap,
                                          int npoints, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs,
                                          const int32_t* d_kf_order, const uint8_t* d_kf_id0, int nlist, const int32_t* d_list, int th,
                                          int conn_cap, int32_t* d_conn_kf, int32_t* d_conn_w, int32_t* d_nconn, int32_t* d_ord_kf, int32_t* d_ord_w,
                                          int32_t* d_nord, int32_t* d_parent, uint8_t* d_first_connection, int32_t* d_row_status,
                                          int loop_conn_cap, int32_t* d_loop_conn, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || nlist < 0 || th < 1 || conn_cap < 1 || loop_conn_cap < 0 || !d_info ||
        (nframes && (!d_kf_point || !d_n || !d_conn_kf || !d_conn_w || !d_nconn || !d_ord_kf || !d_ord_w || !d_nord || !d_parent ||
                     !d_first_connection || !d_row_status)) ||
        (npoints && !d_obs_start) || (nobs && !d_obs_frame) || (nlist && !d_list) || (loop_conn_cap && !d_loop_conn))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_update_connections_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    if (nlist > nframes) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections_batch_device: the list is longer than the batch");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const int nf = std::max(nframes, 1), nl = std::max(nlist, 1);
    const size_t oPos = 0, oInv = oPos + (size_t)nf * 4, oMeta = oInv + (size_t)nf * 4, oLc = oMeta + (size_t)nl * 16,
                 oW = oLc + (size_t)nl * 4, oFlag = oW + (size_t)nl * nf * 4, end = oFlag + (size_t)nl * conn_cap;
    void* scr;
    int rc = pg_ctx_scratch(c, end, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    PgCovBatch B = {d_kf_point, d_n, nframes, cap, npoints, d_point_bad, d_obs_start, d_obs_frame, nobs, d_kf_order, d_kf_id0, nlist, d_list, th,
                    conn_cap, d_conn_kf, d_conn_w, d_nconn, d_ord_kf, d_ord_w, d_nord, d_parent, d_first_connection, d_row_status,
                    d_loop_conn ? loop_conn_cap : 0, d_loop_conn, d_info,
                    (int32_t*)(b + oPos), (int32_t*)(b + oInv), (int32_t*)(b + oMeta), (int32_t*)(b + oLc), (int32_t*)(b + oW), b + oFlag};
    if (hipMemsetAsync(b, 0xFF, oMeta, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    if (nframes) {
        hipLaunchKernelGGL(k_cov_prep, dim3((unsigned)((nf + COV_T - 1) / COV_T)), dim3(COV_T), 0, s, d_kf_order, nframes, d_list, nlist, B.inv, B.pos);
        if (nlist) hipLaunchKernelGGL(k_cov_count, dim3((unsigned)nlist), dim3(COV_T), 0, s, B);
        hipLaunchKernelGGL(k_cov_finish, dim3((unsigned)nframes), dim3(COV_T), 0, s, B);
    }
    hipLaunchKernelGGL(k_cov_loop, dim3((unsigned)nl), dim3(COV_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cov_prep / k_cov_count / k_cov_finish / k_cov_loop launch failed");
    return pg_ctx_scratch_done(c, s);
}

int pgorb_covisibility_views_device(pgorb_ctx* c, int nframes, int conn_cap, const int32_t* d_ord_kf, const int32_t* d_ord_w, const int32_t* d_nord,
                                    int nbest, int32_t* d_best, int ncovis_cap, int32_t* d_covis_start, int32_t* d_covis, int32_t* d_covis_weight,
                                    int w, int32_t* d_by_weight, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || conn_cap < 1 || nbest < 0 || ncovis_cap < 0 || !d_info || (nframes && (!d_ord_kf || !d_ord_w || !d_nord)) ||
        (d_best && nbest < 1) || (d_covis_start && ncovis_cap && (!d_covis || !d_covis_weight)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_covisibility_views_device");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    if (!nframes) {
        if (hipMemsetAsync(d_info, 0, 8, s) != hipSuccess || (d_covis_start && hipMemsetAsync(d_covis_start, 0, 4, s) != hipSuccess))
            return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
        return 0;
    }
    hipLaunchKernelGGL(k_cov_views, dim3((unsigned)nframes), dim3(64), 0, s, nframes, conn_cap, d_ord_kf, d_ord_w, d_nord, nbest, d_best, ncovis_cap,
                       d_covis_start, d_covis, d_covis_weight, w, d_by_weight, d_info);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cov_views launch failed");
    return 0;
}

int pgorb_update_local_map_batch_device(pgorb_ctx* c, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap, const uint8_t* d_kf_bad,
                                        const int32_t* d_pair_frame, int npairs, const int32_t* d_kp_point,
                                        int npoints, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs,
                                        int conn_cap, const int32_t* d_ord_kf, const int32_t* d_nord, const int32_t* d_parent, const int32_t* d_kf_order,
                                        int nbest, int max_local, int lkf_cap, const int32_t* d_prev_local_kf, const int32_t* d_nprev,
                                        int32_t* d_kp_point_out, int32_t* d_local_kf, int32_t* d_nlocal_kf, int32_t* d_ref_kf,
                                        int qcap, int32_t* d_queries, int32_t* d_nq, int32_t* d_status, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npairs < 0 || npoints < 0 || nobs < 0 || conn_cap < 1 || nbest < 0 || max_local < 0 || lkf_cap < 1 || qcap < 1 ||
        (nframes && (!d_kf_point || !d_n || !d_ord_kf || !d_nord || !d_parent)) || (npoints && !d_obs_start) || (nobs && !d_obs_frame) ||
        (npairs && (!d_kp_point || !d_local_kf || !d_nlocal_kf || !d_ref_kf || !d_queries || !d_nq || !d_status)) ||
        (!d_pair_frame && npairs > nframes) || ((d_prev_local_kf != nullptr) != (d_nprev != nullptr)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_update_local_map_batch_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (qcap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "qcap above 16000");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    if (lkf_cap > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "lkf_cap above PGORB_COVIS_MAX_KF");
    if ((uint64_t)lkf_cap * (uint64_t)cap > 0xFFFFFFFEull) return pg_ctx_fail(c, PGORB_E_LIMIT, "lkf_cap * cap_per_frame does not fit 32 bits");
    if (!npairs) return 0;
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const int nf = std::max(nframes, 1);
    const size_t oInv = 0, oFirst = ((size_t)nf * 4 + 63) & ~(size_t)63, end = oFirst + (size_t)npairs * std::max(npoints, 1) * 4;
    void* scr;
    int rc = pg_ctx_scratch(c, end, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    if (hipMemsetAsync(b, 0xFF, end, s) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    PgLocalMapBatch B = {d_kf_point, d_n, nframes, cap, d_kf_bad, d_pair_frame, npairs, d_kp_point, npoints, d_point_bad, d_obs_start, d_obs_frame, nobs,
                         conn_cap, d_ord_kf, d_nord, d_parent, d_kf_order, nbest, max_local, lkf_cap, d_prev_local_kf, d_nprev,
                         d_kp_point_out, d_local_kf, d_nlocal_kf, d_ref_kf, qcap, d_queries, d_nq, d_status, (const int32_t*)(b + oInv), (unsigned*)(b + oFirst)};
    if (nframes)
        hipLaunchKernelGGL(k_cov_prep, dim3((unsigned)((nf + COV_T - 1) / COV_T)), dim3(COV_T), 0, s, d_kf_order, nframes, (const int32_t*)nullptr, 0,
                           (int32_t*)(b + oInv), (int32_t*)nullptr);
    hipLaunchKernelGGL(k_cov_local, dim3((unsigned)npairs), dim3(COV_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cov_prep / k_cov_local launch failed");
    return pg_ctx_scratch_done(c, s);
}

// the table's observation lists, as the single calls require them
static int cov_check_table(pgorb_ctx* c, const char* fn, int nkf, int npoints, const int32_t* obs_start, const int32_t* obs_frame, std::string& msg)
{
    if (npoints && !obs_start) { msg = std::string("bad argument to ") + fn; return PGORB_E_ARG; }
    if (!npoints) return 0;
    if (obs_start[0] != 0) { msg = std::string(fn) + ": obs_start[0] must be 0"; return PGORB_E_ARG; }
    for (int i = 0; i < npoints; i++)
        if (obs_start[i + 1] < obs_start[i]) { msg = std::string(fn) + ": obs_start decreases"; return PGORB_E_ARG; }
    const int nobs = obs_start[npoints];
    if (nobs && !obs_frame) { msg = std::string("bad argument to ") + fn; return PGORB_E_ARG; }
    std::vector<int32_t> seen((size_t)std::max(nkf, 1), -1);
    for (int i = 0; i < npoints; i++)
        for (int k = obs_start[i]; k < obs_start[i + 1]; k++) {
            if (obs_frame[k] < 0 || obs_frame[k] >= nkf) { msg = std::string(fn) + ": an observation names a key frame out of range"; return PGORB_E_ARG; }
            if (seen[obs_frame[k]] == i) { msg = std::string(fn) + ": a list names a key frame twice"; return PGORB_E_ARG; }
            seen[obs_frame[k]] = i;
        }
    return 0;
}
static bool cov_is_permutation(const int32_t* order, int n)
{
    if (!order) return true;
    std::vector<uint8_t> seen((size_t)std::max(n, 1), 0);
    for (int f = 0; f < n; f++) {
        if (order[f] < 0 || order[f] >= n || seen[order[f]]) return false;
        seen[order[f]] = 1;
    }
    return true;
}

int pgorb_update_connections(pgorb_ctx* c, int nkf, const int32_t* const* kf_point, const int32_t* n, int npoints, const uint8_t* point_bad,
                             const int32_t* obs_start, const int32_t* obs_frame, const int32_t* kf_order, const uint8_t* kf_id0,
                             int nlist, const int32_t* list, int th, int conn_cap, int32_t* conn_kf, int32_t* conn_w, int32_t* nconn,
                             int32_t* ord_kf, int32_t* ord_w, int32_t* nord, int32_t* parent, uint8_t* first_connection, int32_t* row_status,
                             int loop_conn_cap, int32_t* loop_conn, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* fn = "pgorb_update_connections";
    const char* bad = "bad argument to pgorb_update_connections";
    if (nkf < 0 || npoints < 0 || nlist < 0 || th < 1 || conn_cap < 1 || loop_conn_cap < 0 || !info || (loop_conn_cap && !loop_conn) ||
        (nkf && (!kf_point || !n || !conn_kf || !conn_w || !nconn || !ord_kf || !ord_w || !nord || !parent || !first_connection || !row_status)) ||
        (nlist && !list))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (nkf > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    int cap = 1;
    for (int f = 0; f < nkf; f++) {
        if (n[f] < 0 || (n[f] && !kf_point[f])) return pg_ctx_fail(c, PGORB_E_ARG, bad);
        if (n[f] > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        cap = std::max(cap, n[f]);
        for (int s = 0; s < n[f]; s++)
            if (kf_point[f][s] < -1 || kf_point[f][s] >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a slot names a point out of range");
    }
    std::string msg;
    if (cov_check_table(c, fn, nkf, npoints, obs_start, obs_frame, msg)) return pg_ctx_fail(c, PGORB_E_ARG, msg.c_str());
    if (!cov_is_permutation(kf_order, nkf)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: kf_order is not a permutation");
    {
        std::vector<uint8_t> seen((size_t)std::max(nkf, 1), 0);
        for (int k = 0; k < nlist; k++) {
            if (list[k] < 0 || list[k] >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a list entry is out of range");
            if (seen[list[k]]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: the list names a key frame twice");
            seen[list[k]] = 1;
        }
        std::vector<int32_t> mark((size_t)std::max(nkf, 1), -1);
        for (int f = 0; f < nkf; f++) {
            if (nconn[f] < 0 || nconn[f] > conn_cap || nord[f] < 0 || nord[f] > conn_cap)
                return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a row count is outside [0, conn_cap]");
            if (parent[f] < -1 || parent[f] >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a parent is out of range");
            int last = -1;
            for (int t = 0; t < nconn[f]; t++) {
                const int j = conn_kf[(size_t)f * conn_cap + t];
                if (j < 0 || j >= nkf || j == f) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a connection is out of range");
                const int r = kf_order ? kf_order[j] : j;
                if (r <= last) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: a connection row is not in address order");
                last = r;
                mark[j] = f;
            }
            for (int t = 0; t < nord[f]; t++) {
                const int j = ord_kf[(size_t)f * conn_cap + t];
                if (j < 0 || j >= nkf || mark[j] != f) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_connections: an ordered entry is not in the row's map");
            }
        }
    }
    const int nf = std::max(nkf, 1), np = std::max(npoints, 1), nobs = npoints ? obs_start[npoints] : 0, no = std::max(nobs, 1);
    const size_t rowB = (size_t)nf * conn_cap * 4;
    PgHostCall hc(c);
    const size_t oS = hc.region(PG_UP, (size_t)nf * cap * 4), oN = hc.region(PG_UP, (size_t)nf * 4), oB = hc.region(PG_UP, np),
                 oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = hc.region(PG_UP, (size_t)no * 4), oOrd = hc.region(PG_UP, (size_t)nf * 4),
                 oId0 = hc.region(PG_UP, nf), oL = hc.region(PG_UP, (size_t)std::max(nlist, 1) * 4),
                 oCK = hc.region(PG_INOUT, rowB), oCW = hc.region(PG_INOUT, rowB), oNC = hc.region(PG_INOUT, (size_t)nf * 4),
                 oOK = hc.region(PG_INOUT, rowB), oOW = hc.region(PG_INOUT, rowB), oNO = hc.region(PG_INOUT, (size_t)nf * 4),
                 oPar = hc.region(PG_INOUT, (size_t)nf * 4), oFirst = hc.region(PG_INOUT, nf),
                 oSt = hc.region(PG_DOWN, (size_t)nf * 4), oLoop = hc.region(PG_DOWN, (size_t)std::max(loop_conn_cap, 1) * 12),
                 oInfo = hc.region(PG_DOWN, PGORB_COVIS_INFO * 4);
    int rc = hc.begin();
    if (rc) return rc;
    for (int f = 0; f < nf; f++) {
        int32_t* row = hc.host<int32_t>(oS) + (size_t)f * cap;
        const int m = f < nkf ? n[f] : 0;
        for (int s = 0; s < cap; s++) row[s] = s < m ? kf_point[f][s] : -1;
    }
    hc.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oB, point_bad, npoints, 0, np);
    if (npoints) hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4); else hc.put(oOS, nullptr, 0, 0, 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOrd, kf_order, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oId0, kf_id0, nkf, 0, nf);
    hc.put(oL, list, (size_t)nlist * 4, 0, (size_t)std::max(nlist, 1) * 4);
    hc.put(oCK, conn_kf, (size_t)nkf * conn_cap * 4, 0, rowB);
    hc.put(oCW, conn_w, (size_t)nkf * conn_cap * 4, 0, rowB);
    hc.put(oNC, nconn, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oOK, ord_kf, (size_t)nkf * conn_cap * 4, 0, rowB);
    hc.put(oOW, ord_w, (size_t)nkf * conn_cap * 4, 0, rowB);
    hc.put(oNO, nord, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oPar, parent, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oFirst, first_connection, nkf, 0, nf);
    if ((rc = hc.run([&] {
            return pgorb_update_connections_batch_device(c, hc.dev<int32_t>(oS), hc.dev<int32_t>(oN), nkf, cap, npoints, hc.dev(oB), hc.dev<int32_t>(oOS),
                                                         hc.dev<int32_t>(oOF), nobs, kf_order ? hc.dev<int32_t>(oOrd) : nullptr, hc.dev(oId0), nlist,
                                                         hc.dev<int32_t>(oL), th, conn_cap, hc.dev<int32_t>(oCK), hc.dev<int32_t>(oCW), hc.dev<int32_t>(oNC),
                                                         hc.dev<int32_t>(oOK), hc.dev<int32_t>(oOW), hc.dev<int32_t>(oNO), hc.dev<int32_t>(oPar),
                                                         hc.dev(oFirst), hc.dev<int32_t>(oSt), loop_conn_cap, loop_conn_cap ? hc.dev<int32_t>(oLoop) : nullptr,
                                                         hc.dev<int32_t>(oInfo), nullptr); }))) return rc;
    memcpy(conn_kf, hc.host(oCK), (size_t)nkf * conn_cap * 4);
    memcpy(conn_w, hc.host(oCW), (size_t)nkf * conn_cap * 4);
    memcpy(nconn, hc.host(oNC), (size_t)nkf * 4);
    memcpy(ord_kf, hc.host(oOK), (size_t)nkf * conn_cap * 4);
    memcpy(ord_w, hc.host(oOW), (size_t)nkf * conn_cap * 4);
    memcpy(nord, hc.host(oNO), (size_t)nkf * 4);
    memcpy(parent, hc.host(oPar), (size_t)nkf * 4);
    memcpy(first_connection, hc.host(oFirst), nkf);
    memcpy(row_status, hc.host(oSt), (size_t)nkf * 4);
    if (loop_conn_cap) memcpy(loop_conn, hc.host(oLoop), (size_t)loop_conn_cap * 12);
    memcpy(info, hc.host(oInfo), PGORB_COVIS_INFO * 4);
    int updated = 0;
    for (int f = 0; f < nkf; f++) updated += (row_status[f] & PGORB_COVIS_UPDATED) != 0;
    return updated;
}

int pgorb_update_local_map(pgorb_ctx* c, int nkf, const int32_t* const* kf_point, const int32_t* n, const uint8_t* kf_bad,
                           const int32_t* kp_point, int nkp, int npoints, const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame,
                           int conn_cap, const int32_t* ord_kf, const int32_t* nord, const int32_t* parent, const int32_t* kf_order,
                           int nbest, int max_local, int nprev, const int32_t* prev_local_kf,
                           int32_t* kp_point_out, int lkf_cap, int32_t* local_kf, int32_t* nlocal_kf, int32_t* ref_kf,
                           int qcap, int32_t* queries, int32_t* nq, int32_t* status)
{
    if (!c) return PGORB_E_ARG;
    const char* fn = "pgorb_update_local_map";
    const char* bad = "bad argument to pgorb_update_local_map";
    if (nkf < 0 || nkp < 0 || npoints < 0 || conn_cap < 1 || nbest < 0 || max_local < 0 || nprev < -1 || lkf_cap < 1 || qcap < 1 ||
        (nkf && (!kf_point || !n || !ord_kf || !nord || !parent)) || (nkp && !kp_point) || (nprev > 0 && !prev_local_kf) ||
        !local_kf || !nlocal_kf || !ref_kf || !queries || !nq || !status)
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (nkf + 1 > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF - 1 key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    if (lkf_cap > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "lkf_cap above PGORB_COVIS_MAX_KF");
    if (qcap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "qcap above 16000");
    if (nkp > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
    if (nprev > lkf_cap) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: the previous list is longer than lkf_cap");
    int cap = std::max(nkp, 1);
    for (int f = 0; f < nkf; f++) {
        if (n[f] < 0 || (n[f] && !kf_point[f])) return pg_ctx_fail(c, PGORB_E_ARG, bad);
        if (n[f] > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        cap = std::max(cap, n[f]);
        for (int s = 0; s < n[f]; s++)
            if (kf_point[f][s] < -1 || kf_point[f][s] >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: a slot names a point out of range");
        if (nord[f] < 0 || nord[f] > conn_cap) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: a row count is outside [0, conn_cap]");
        for (int t = 0; t < nord[f]; t++)
            if (ord_kf[(size_t)f * conn_cap + t] < 0 || ord_kf[(size_t)f * conn_cap + t] >= nkf)
                return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: an ordered entry is out of range");
        if (parent[f] < -1 || parent[f] >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: a parent is out of range");
    }
    for (int s = 0; s < nkp; s++)
        if (kp_point[s] < -1 || kp_point[s] >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: a slot names a point out of range");
    for (int t = 0; t < nprev; t++)
        if (prev_local_kf[t] < 0 || prev_local_kf[t] >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: a previous key frame is out of range");
    std::string msg;
    if (cov_check_table(c, fn, nkf, npoints, obs_start, obs_frame, msg)) return pg_ctx_fail(c, PGORB_E_ARG, msg.c_str());
    if (!cov_is_permutation(kf_order, nkf)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_update_local_map: kf_order is not a permutation");
    // the batch: the key frames, then the frame itself as frame nkf (it is no key frame: nothing names it, its rank is the last)
    const int nfr = nkf + 1, np = std::max(npoints, 1), nobs = npoints ? obs_start[npoints] : 0, no = std::max(nobs, 1);
    const size_t rowB = (size_t)nfr * conn_cap * 4;
    PgHostCall hc(c);
    const size_t oS = hc.region(PG_UP, (size_t)nfr * cap * 4), oN = hc.region(PG_UP, (size_t)nfr * 4), oKB = hc.region(PG_UP, nfr),
                 oPF = hc.region(PG_UP, 4), oKP = hc.region(PG_UP, (size_t)cap * 4), oB = hc.region(PG_UP, np),
                 oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = hc.region(PG_UP, (size_t)no * 4),
                 oOK = hc.region(PG_UP, rowB), oNO = hc.region(PG_UP, (size_t)nfr * 4), oPar = hc.region(PG_UP, (size_t)nfr * 4),
                 oOrd = hc.region(PG_UP, (size_t)nfr * 4), oPrev = hc.region(PG_UP, (size_t)lkf_cap * 4), oNP = hc.region(PG_UP, 4),
                 oKO = hc.region(PG_DOWN, (size_t)cap * 4), oLK = hc.region(PG_DOWN, (size_t)lkf_cap * 4), oQ = hc.region(PG_DOWN, (size_t)qcap * 4),
                 oOut = hc.region(PG_DOWN, 16);
    int rc = hc.begin();
    if (rc) return rc;
    for (int f = 0; f < nfr; f++) {
        int32_t* row = hc.host<int32_t>(oS) + (size_t)f * cap;
        const int m = f < nkf ? n[f] : 0;
        for (int s = 0; s < cap; s++) row[s] = s < m ? kf_point[f][s] : -1;
        hc.host<int32_t>(oN)[f] = f < nkf ? n[f] : nkp;
        hc.host(oKB)[f] = f < nkf && kf_bad ? kf_bad[f] : 0;
        hc.host<int32_t>(oNO)[f] = f < nkf ? nord[f] : 0;
        hc.host<int32_t>(oPar)[f] = f < nkf ? parent[f] : -1;
        hc.host<int32_t>(oOrd)[f] = f < nkf ? (kf_order ? kf_order[f] : f) : nkf;
    }
    hc.host<int32_t>(oPF)[0] = nkf;
    for (int s = 0; s < cap; s++) hc.host<int32_t>(oKP)[s] = s < nkp ? kp_point[s] : -1;
    hc.put(oB, point_bad, npoints, 0, np);
    if (npoints) hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4); else hc.put(oOS, nullptr, 0, 0, 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOK, ord_kf, (size_t)nkf * conn_cap * 4, 0, rowB);
    hc.put(oPrev, prev_local_kf, (size_t)std::max(nprev, 0) * 4, 0, (size_t)lkf_cap * 4);
    hc.host<int32_t>(oNP)[0] = std::max(nprev, 0);
    if ((rc = hc.run([&] {
            return pgorb_update_local_map_batch_device(c, hc.dev<int32_t>(oS), hc.dev<int32_t>(oN), nfr, cap, hc.dev(oKB), hc.dev<int32_t>(oPF), 1,
                                                       hc.dev<int32_t>(oKP), npoints, hc.dev(oB), hc.dev<int32_t>(oOS), hc.dev<int32_t>(oOF), nobs,
                                                       conn_cap, hc.dev<int32_t>(oOK), hc.dev<int32_t>(oNO), hc.dev<int32_t>(oPar), hc.dev<int32_t>(oOrd),
                                                       nbest, max_local, lkf_cap, nprev >= 0 ? hc.dev<int32_t>(oPrev) : nullptr,
                                                       nprev >= 0 ? hc.dev<int32_t>(oNP) : nullptr, hc.dev<int32_t>(oKO), hc.dev<int32_t>(oLK),
                                                       hc.dev<int32_t>(oOut), hc.dev<int32_t>(oOut) + 1, qcap, hc.dev<int32_t>(oQ),
                                                       hc.dev<int32_t>(oOut) + 2, hc.dev<int32_t>(oOut) + 3, nullptr); }))) return rc;
    const int32_t* out = hc.host<int32_t>(oOut);
    *nlocal_kf = out[0]; *ref_kf = out[1]; *nq = out[2]; *status = out[3];
    if (kp_point_out) memcpy(kp_point_out, hc.host(oKO), (size_t)nkp * 4);
    memcpy(local_kf, hc.host(oLK), (size_t)std::min(std::max(out[0], 0), lkf_cap) * 4);
    memcpy(queries, hc.host(oQ), (size_t)std::min(std::max(out[2], 0), qcap) * 4);
    return out[2];
}

}  // extern "C"
