// culling.hip -- local mapping's two cullings with the map surgery they trigger, next to the map-point table and the covisibility
// graph, on gfx950.  Integers only (one float division in MapPointCulling), every result exact.
//
// Restates (thirdparty/orb-slam2):
//   LocalMapping::MapPointCulling               src/LocalMapping.cc:170-207
//   LocalMapping::KeyFrameCulling               src/LocalMapping.cc:634-698
//   KeyFrame::SetBadFlag, EraseConnection       src/KeyFrame.cc:556-648, :262-275
//   MapPoint::EraseObservation, SetBadFlag      src/MapPoint.cc:132-158, :172-187
//
// The CSR of the observation lists keeps its shape: an erased observation is a cleared byte of obs_live, and one compaction
// afterwards writes a fresh CSR.
//   k_cull_points         MapPointCulling: a thread per recent point (the points are independent), the surviving list by a ballot scan
//   k_cull_eval           KeyFrameCulling: a workgroup per list member counts nMPs / nRedundantObservations from the input state
//   k_cull_walk           ONE workgroup walks cur_kf's ordered row in list order.  A member's counts can change only through a point
//                         that a culled key frame also held or through one of its own slots being cleared, so it takes k_cull_eval's
//                         counts unless a cull cleared one of its slots or one of its slots holds a point a cull has claimed; then the
//                         whole workgroup counts again from the state as it stands.  For a redundant member SetBadFlag runs to its end: the rows that hold it re-sorted in LDS (bitonic, 64-bit keys), its points'
//                         observations erased (a claim per point: one thread owns a point however many slots hold it), its rows
//                         cleared, the spanning tree repaired round by round with one LDS atomicMax per round
//   k_cull_compact_scan   the live length of every list and its exclusive scan, one workgroup
//   k_cull_compact_copy   a thread per point copies its live entries and re-bases ref_obs
// Inside k_cull_walk the workgroup that writes the global state is the only one that reads it: every write is followed by
// __threadfence_block() and a barrier before the dependent read.
#include "match_common.h"
#include <string>
#include <vector>

#define CULL_T 256

struct PgCullTable {
    int32_t* kfPoint; const int32_t* n; int nframes; int cap;
    int npoints; uint8_t* pbad; const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs; uint8_t* live;
};

// the list of point p as [x, y); empty when the pair is no list
__device__ __forceinline__ int2 cull_range(const PgCullTable& T, int p)
{
    const int a = T.obsStart[p], b = T.obsStart[p + 1];
    return (a < 0 || b < a || b > T.nobs) ? make_int2(0, 0) : make_int2(a, b);
}

// observation o as (key frame, keypoint): false when it is dead or names nothing of the batch
__device__ __forceinline__ bool cull_obs(const PgCullTable& T, int o, int& f, int& i)
{
    if (!T.live[o]) return false;
    f = T.obsFrame[o]; i = T.obsIdx[o];
    if (f < 0 || f >= T.nframes) return false;
    return i >= 0 && i < min(max(T.n[f], 0), T.cap);
}

__device__ __forceinline__ int cull_observations(const PgCullTable& T, int2 r)
{
    int cnt = 0, f, i;
    for (int o = r.x; o < r.y; o++) cnt += cull_obs(T, o, f, i);
    return cnt;
}

// MapPoint::SetBadFlag (MapPoint.cc:172-187): EraseMapPointMatch(idx) of every observer, whatever that slot holds
__device__ __forceinline__ void cull_point_bad(const PgCullTable& T, int p, int2 r, uint8_t* dirty = nullptr)
{
    T.pbad[p] = 1;
    for (int o = r.x; o < r.y; o++) {
        int f, i;
        if (cull_obs(T, o, f, i)) {
            T.kfPoint[(int64_t)f * T.cap + i] = -1;
            if (dirty) dirty[f] = 1;                                               // that key frame's counts are to be taken again
        }
        T.live[o] = 0;
    }
}

// exclusive position of a set flag among the workgroup's CULL_T threads, and the total; every thread calls it
__device__ __forceinline__ int cull_scan(bool flag, int* sWave, int& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();
    if (lane == 0) sWave[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < CULL_T / 64; k++) { if (k < w) base += sWave[k]; total += sWave[k]; }
    return base + __popcll(m & ((1ull << lane) - 1));
}

// ascending bitonic sort of key[0 .. m), m a power of two, by the whole workgroup
__device__ __forceinline__ void cull_sort(unsigned long long* key, int m)
{
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < m; t += CULL_T) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long a = key[t], b = key[x];
                    if (((t & k) == 0) ? (a > b) : (a < b)) { key[t] = b; key[x] = a; }
                }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(CULL_T) void k_cull_points(PgCullTable T, const int32_t* __restrict__ firstKf, const int32_t* __restrict__ visible,
                                                        const int32_t* __restrict__ found, int nrecent, const int32_t* recent, int curKfId, int thObs,
                                                        int32_t* action, int32_t* recentOut, int32_t* nrecentOut, int32_t* info)
{
    __shared__ int sWave[CULL_T / 64];
    __shared__ int sCulled;
    const int tid = threadIdx.x;
    if (tid == 0) sCulled = 0;
    __syncthreads();
    int base = 0;
    for (int t0 = 0; t0 < nrecent; t0 += CULL_T) {
        const int t = t0 + tid;
        int act = PGORB_CULL_MP_NONE, p = -1;
        if (t < nrecent) {
            p = recent[t];
            if (p >= 0 && p < T.npoints) {
                const int2 r = cull_range(T, p);
                const int age = (int)((unsigned)curKfId - (unsigned)firstKf[p]);
                if (T.pbad[p]) act = PGORB_CULL_MP_WAS_BAD;                                                  // :186
                else if (__fdiv_rn((float)found[p], (float)visible[p]) < 0.25f) act = PGORB_CULL_MP_FOUND_RATIO;   // :190
                else if (age >= 2 && cull_observations(T, r) <= thObs) act = PGORB_CULL_MP_FEW_OBS;          // :196
                else if (age >= 3) act = PGORB_CULL_MP_AGED;                                                 // :202
                else act = PGORB_CULL_MP_KEEP;
                if (act == PGORB_CULL_MP_FOUND_RATIO || act == PGORB_CULL_MP_FEW_OBS) {
                    cull_point_bad(T, p, r);
                    atomicAdd(&sCulled, 1);
                }
            }
            action[t] = act;
        }
        int chunk;
        const int at = base + cull_scan(t < nrecent && act == PGORB_CULL_MP_KEEP, sWave, chunk);
        if (t < nrecent && act == PGORB_CULL_MP_KEEP) recentOut[at] = p;
        base += chunk;
    }
    __syncthreads();
    if (tid == 0) { nrecentOut[0] = base; info[0] = 0; info[1] = base; info[2] = sCulled; info[3] = 0; }
}

struct PgCullKf {
    PgCullTable T;
    const pgorb_keypoint* kps; int32_t* refObs;
    const int32_t* order; const uint8_t* id0; const uint8_t* notErase; uint8_t* kfBad; uint8_t* toBeErased; int curKf;
    int connCap; int32_t* connKf; int32_t* connW; int32_t* nconn; int32_t* ordKf; int32_t* ordW; int32_t* nord; int32_t* parent;
    int listCap; int32_t* record; int32_t* rowStatus; int32_t* info;
    int32_t* inv; int32_t* claim; int32_t* pre;                                    // scratch
};

// the address rank of key frame f, or -1 when kf_order gives it none of its own
__device__ __forceinline__ int cull_rank(const PgCullKf& B, int f)
{
    const int r = B.order ? B.order[f] : f;
    return (r >= 0 && r < B.T.nframes && B.inv[r] == f) ? r : -1;
}

struct PgCullLds {
    int32_t list[PGORB_COVIS_MAX_CONN];
    unsigned long long key[PGORB_COVIS_MAX_CONN];
    int32_t tmp[PGORB_COVIS_MAX_KF];                                               // a staged row (key frames, then weights); the children
    uint8_t cand[PGORB_COVIS_MAX_KF];
    uint8_t dirty[PGORB_COVIS_MAX_KF];                                             // a cull cleared one of this key frame's slots
    unsigned long long best;
    int wave[CULL_T / 64];
    int a, b, pos, wentBad;                                                        // a and b stay adjacent: cull_count takes &a as its pair
};
static_assert(PGORB_COVIS_MAX_KF >= 2 * PGORB_COVIS_MAX_CONN, "a staged row needs two halves of PgCullLds::tmp");

// KeyFrameCulling's counts of member A (LocalMapping.cc:646-691) from the state as it stands; every thread calls it
__device__ void cull_count(const PgCullKf& B, int* sAB /* LDS [2] */, int A, int& nmp, int& red)
{
    const PgCullTable& T = B.T;
    const int tid = threadIdx.x;
    if (tid == 0) { sAB[0] = 0; sAB[1] = 0; }
    __syncthreads();
    const int n = min(max(T.n[A], 0), T.cap);
    int m = 0, r = 0;
    for (int s = tid; s < n; s += CULL_T) {
        const int p = T.kfPoint[(int64_t)A * T.cap + s];
        if (p < 0 || p >= T.npoints || T.pbad[p]) continue;
        m++;
        const long long lvl = B.kps[(int64_t)A * T.cap + s].octave;
        const int2 q = cull_range(T, p);
        int all = 0, fine = 0;
        for (int o = q.x; o < q.y; o++) {
            int f, i;
            if (!cull_obs(T, o, f, i)) continue;
            all++;
            if (f != A && (long long)B.kps[(int64_t)f * T.cap + i].octave <= lvl + 1) fine++;   // the break at :682 does not change fine >= 3
        }
        r += all > 3 && fine >= 3;
    }
    if (m) atomicAdd(&sAB[0], m);
    if (r) atomicAdd(&sAB[1], r);
    __syncthreads();
    nmp = sAB[0]; red = sAB[1];
    __syncthreads();
}

// does a slot of A hold a point that a cull has claimed (its list or its bad flag changed)?  every thread calls it
__device__ bool cull_touched(const PgCullKf& B, PgCullLds& S, int A)
{
    const PgCullTable& T = B.T;
    if (threadIdx.x == 0) S.pos = 0;
    __syncthreads();
    const int n = min(max(T.n[A], 0), T.cap);
    bool any = false;
    for (int s = threadIdx.x; s < n && !any; s += CULL_T) {
        const int p = T.kfPoint[(int64_t)A * T.cap + s];
        any = p >= 0 && p < T.npoints && B.claim[p] != 0;
    }
    if (any) S.pos = 1;
    __syncthreads();
    const bool r = S.pos != 0;
    __syncthreads();
    return r;
}

// the list: cur_kf's ordered row as it stands; its length, or -1 when it is longer than list_cap
__device__ __forceinline__ int cull_list_length(const PgCullKf& B)
{
    const int cur = B.curKf;
    const int nl = (cur >= 0 && cur < B.T.nframes) ? min(max(B.nord[cur], 0), B.connCap) : 0;
    return nl > B.listCap ? -1 : nl;
}

__global__ __launch_bounds__(CULL_T) void k_cull_eval(PgCullKf B)
{
    __shared__ int sAB[2];
    const int t = blockIdx.x;
    if (t >= cull_list_length(B)) return;
    const int A = B.ordKf[(int64_t)B.curKf * B.connCap + t];
    if (A < 0 || A >= B.T.nframes || (B.id0 && B.id0[A])) return;
    int nmp, red;
    cull_count(B, sAB, A, nmp, red);
    if (threadIdx.x == 0) { B.pre[2 * t] = nmp; B.pre[2 * t + 1] = red; }
}

// EraseConnection(A) on row j (KeyFrame.cc:262-275): the entry leaves the map, UpdateBestCovisibles rebuilds the list from the whole map
__device__ void cull_erase_connection(const PgCullKf& B, PgCullLds& S, int j, int A)
{
    const int tid = threadIdx.x, nf = B.T.nframes, half = PGORB_COVIS_MAX_CONN;
    const int64_t row = (int64_t)j * B.connCap;
    const int nc = min(max(B.nconn[j], 0), B.connCap), noOld = min(max(B.nord[j], 0), B.connCap);
    if (tid == 0) { S.pos = -1; S.a = 0; }
    __syncthreads();
    for (int t = tid; t < nc; t += CULL_T) {
        const int f = B.connKf[row + t];
        S.tmp[t] = f; S.tmp[half + t] = B.connW[row + t];
        if (f == A) atomicMax(&S.pos, t);
    }
    __syncthreads();
    const int pos = S.pos;
    if (pos < 0) { __syncthreads(); return; }
    const int m = nc - 1;
    int m2 = 1;
    while (m2 < m) m2 <<= 1;
    for (int t = tid; t < m2; t += CULL_T) S.key[t] = ~0ull;
    for (int t = tid; t < m; t += CULL_T) {
        const int src = t < pos ? t : t + 1;
        B.connKf[row + t] = S.tmp[src]; B.connW[row + t] = S.tmp[half + src];
    }
    __syncthreads();
    for (int t = tid; t < nc; t += CULL_T) {
        const int f = S.tmp[t];
        if (t == pos || f < 0 || f >= nf) continue;
        const int r = cull_rank(B, f);
        if (r < 0) continue;
        const unsigned long long key = ((unsigned long long)((unsigned)S.tmp[half + t] ^ 0x80000000u) << 32) | (unsigned)r;
        S.key[atomicAdd(&S.a, 1)] = ~key;
    }
    cull_sort(S.key, m2);
    const int no = S.a;
    for (int t = tid; t < max(no, noOld); t += CULL_T) {
        const unsigned long long key = ~S.key[min(t, PGORB_COVIS_MAX_CONN - 1)];
        B.ordKf[row + t] = t < no ? B.inv[(int)(unsigned)(key & 0xFFFFFFFFu)] : -1;
        B.ordW[row + t] = t < no ? (int)((unsigned)(key >> 32) ^ 0x80000000u) : 0;
    }
    if (tid == 0) {
        B.connKf[row + m] = -1; B.connW[row + m] = 0;
        B.nconn[j] = m; B.nord[j] = no;
        B.rowStatus[j] |= PGORB_CULL_ROW_ERASED;
    }
    __threadfence_block();
    __syncthreads();
}

// KeyFrame::SetBadFlag of A past its two early returns (KeyFrame.cc:569-646); stamp > 0 is this cull's own
__device__ void cull_set_bad_flag(const PgCullKf& B, PgCullLds& S, int A, int stamp)
{
    const PgCullTable& T = B.T;
    const int tid = threadIdx.x, nf = T.nframes;
    const int64_t rowA = (int64_t)A * B.connCap;
    const int ncA = min(max(B.nconn[A], 0), B.connCap), noA = min(max(B.nord[A], 0), B.connCap);
    for (int e = 0; e < ncA; e++) {                                                // :569-570, in address order; row A itself does not change here
        const int j = B.connKf[rowA + e];
        if (j < 0 || j >= nf || j == A || cull_rank(B, j) < 0) continue;
        cull_erase_connection(B, S, j, A);
    }
    const int n = min(max(T.n[A], 0), T.cap);
    int went = 0;
    for (int s = tid; s < n; s += CULL_T) {                                        // :572-574; A's own slots keep their values
        const int p = T.kfPoint[(int64_t)A * T.cap + s];
        if (p < 0 || p >= T.npoints) continue;
        if (atomicMax(&B.claim[p], stamp) >= stamp) continue;                      // a second slot with p: mObservations.count(pKF) is 0 by then
        const int2 q = cull_range(T, p);
        int at = -1, f, i;
        for (int o = q.x; o < q.y && at < 0; o++)
            if (cull_obs(T, o, f, i) && f == A) at = o;
        if (at < 0) continue;
        T.live[at] = 0;                                                            // MapPoint::EraseObservation (MapPoint.cc:132-158)
        if (B.refObs[p] == at - q.x) {                                             // mpRefKF = mObservations.begin()->first; none left: -1
            int first = -1;
            for (int o = q.x; o < q.y && first < 0; o++)
                if (cull_obs(T, o, f, i)) first = o - q.x;
            B.refObs[p] = first;
        }
        if (cull_observations(T, q) <= 2) {
            went += !T.pbad[p];
            cull_point_bad(T, p, q, S.dirty);
        }
    }
    if (went) atomicAdd(&S.wentBad, went);
    for (int t = tid; t < ncA; t += CULL_T) { B.connKf[rowA + t] = -1; B.connW[rowA + t] = 0; }   // :579-580
    for (int t = tid; t < noA; t += CULL_T) { B.ordKf[rowA + t] = -1; B.ordW[rowA + t] = 0; }
    for (int f = tid; f < nf; f += CULL_T) S.cand[f] = 0;
    __threadfence_block();
    __syncthreads();
    const int pa = B.parent[A];
    const int paOk = pa >= 0 && pa < nf ? pa : -1;
    if (tid == 0) {
        B.nconn[A] = 0; B.nord[A] = 0;
        B.rowStatus[A] |= PGORB_CULL_ROW_CLEARED;
        if (paOk >= 0) S.cand[paOk] = 1;                                           // sParentCandidates = {mpParent} (:584)
    }
    int nch = 0;
    for (int r0 = 0; r0 < nf; r0 += CULL_T) {                                      // mspChildrens without the bad ones (:599), in address order
        const int r = r0 + tid;
        const int f = r < nf ? B.inv[r] : -1;
        const bool in = f >= 0 && f != A && B.parent[f] == A && !B.kfBad[f] && cull_rank(B, f) == r;
        int chunk;
        const int at = nch + cull_scan(in, S.wave, chunk);
        if (in) S.tmp[at] = f;
        nch += chunk;
    }
    __syncthreads();
    for (;;) {                                                                     // :588-632
        if (tid == 0) S.best = 0;
        __syncthreads();
        for (int ci = 0; ci < nch; ci++) {
            const int c = S.tmp[ci];
            if (c < 0) continue;
            const int64_t rowC = (int64_t)c * B.connCap;
            const int no = min(max(B.nord[c], 0), B.connCap), nc = min(max(B.nconn[c], 0), B.connCap);
            for (int i = tid; i < no; i += CULL_T) {
                const int x = B.ordKf[rowC + i];
                if (x < 0 || x >= nf || !S.cand[x]) continue;
                int w = 0;                                                         // GetWeight: 0 when the map does not hold it
                for (int t = 0; t < nc; t++)
                    if (B.connKf[rowC + t] == x) { w = B.connW[rowC + t]; break; }
                if (w < 0) continue;                                               // w > max, max = -1
                atomicMax(&S.best, ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7FFFFFFF - (ci * PGORB_COVIS_MAX_CONN + i)));
            }
        }
        __syncthreads();
        const unsigned long long best = S.best;
        __syncthreads();
        if (!best) break;
        const int lo = 0x7FFFFFFF - (int)(unsigned)(best & 0xFFFFFFFFu);
        const int ci = lo / PGORB_COVIS_MAX_CONN, i = lo % PGORB_COVIS_MAX_CONN;
        if (tid == 0) {                                                            // the first strict maximum: ChangeParent, a new candidate
            const int c = S.tmp[ci];
            B.parent[c] = B.ordKf[(int64_t)c * B.connCap + i];
            B.rowStatus[c] |= PGORB_CULL_ROW_REPARENTED;
            S.cand[c] = 1;
            S.tmp[ci] = -1;
        }
        __threadfence_block();
        __syncthreads();
    }
    for (int ci = tid; ci < nch; ci += CULL_T) {                                   // :635-639; parent[A] itself keeps its value
        const int c = S.tmp[ci];
        if (c >= 0) { B.parent[c] = paOk; B.rowStatus[c] |= PGORB_CULL_ROW_REPARENTED; }
    }
    if (tid == 0) B.kfBad[A] = 1;
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(CULL_T) void k_cull_walk(PgCullKf B)
{
    __shared__ PgCullLds S;
    const int tid = threadIdx.x, nf = B.T.nframes;
    for (int f = tid; f < nf; f += CULL_T) {
        const int r = B.order ? B.order[f] : f;
        if (r >= 0 && r < nf) atomicMax(&B.inv[r], f);                             // a rank named twice belongs to the larger index
    }
    __threadfence_block();
    __syncthreads();
    const int cur = B.curKf;
    const int nl = cull_list_length(B);
    if (nl < 0) {
        if (tid == 0) { B.info[0] = PGORB_CULL_LIMIT; B.info[1] = min(max(B.nord[cur], 0), B.connCap); B.info[2] = 0; B.info[3] = 0; }
        return;
    }
    for (int t = tid; t < nl; t += CULL_T) S.list[t] = B.ordKf[(int64_t)cur * B.connCap + t];   // the copy of :640
    for (int f = tid; f < nf; f += CULL_T) { B.rowStatus[f] = 0; S.dirty[f] = 0; }
    if (tid == 0) S.wentBad = 0;
    __threadfence_block();
    __syncthreads();
    int culled = 0;
    for (int t = 0; t < nl; t++) {
        const int A = S.list[t];
        int act, nmp = -1, red = -1;
        if (A < 0 || A >= nf || cull_rank(B, A) < 0) act = PGORB_CULL_KF_NONE;
        else if (B.id0 && B.id0[A]) act = PGORB_CULL_KF_ID0;                        // :645
        else {
            bool again = culled > 0;                                               // nothing culled yet: the input state still stands
            if (again) again = S.dirty[A] || cull_touched(B, S, A);
            if (again) cull_count(B, &S.a, A, nmp, red);
            else { nmp = B.pre[2 * t]; red = B.pre[2 * t + 1]; }
            const bool redundant = (double)red > 0.9 * (double)nmp;                // :694
            if (B.kfBad[A]) act = PGORB_CULL_KF_WAS_BAD;
            else if (!redundant) act = PGORB_CULL_KF_KEEP;
            else if (B.notErase && B.notErase[A]) {                                // KeyFrame.cc:562-566
                act = PGORB_CULL_KF_TO_BE_ERASED;
                if (tid == 0 && B.toBeErased) B.toBeErased[A] = 1;
            } else {
                act = PGORB_CULL_KF_CULLED;
                culled++;
                cull_set_bad_flag(B, S, A, t + 1);
            }
        }
        if (tid == 0) { int32_t* rec = B.record + 4 * (int64_t)t; rec[0] = A; rec[1] = nmp; rec[2] = red; rec[3] = act; }
    }
    __syncthreads();
    if (tid == 0) { B.info[0] = 0; B.info[1] = nl; B.info[2] = culled; B.info[3] = S.wentBad; }
}

__global__ __launch_bounds__(CULL_T) void k_cull_compact_scan(int npoints, const int32_t* __restrict__ obsStart, int nobs, const uint8_t* __restrict__ live,
                                                              int32_t* __restrict__ startOut, int32_t* __restrict__ info)
{
    __shared__ int32_t part[CULL_T + 1];
    const int t = threadIdx.x;
    const int chunk = (npoints + CULL_T - 1) / CULL_T, k0 = min(t * chunk, npoints), k1 = min(k0 + chunk, npoints);
    int s = 0;
    for (int p = k0; p < k1; p++) {
        const int a = obsStart[p], b = obsStart[p + 1];
        int cnt = 0;
        if (a >= 0 && b >= a && b <= nobs)
            for (int o = a; o < b; o++) cnt += live[o] != 0;
        startOut[p] = cnt;
        s += cnt;
    }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < CULL_T; k++) { const int v = part[k]; part[k] = run; run += v; }
        part[CULL_T] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int p = k0; p < k1; p++) { const int v = startOut[p]; startOut[p] = run; run += v; }
    if (t == 0) { startOut[npoints] = part[CULL_T]; info[0] = part[CULL_T]; }
}

__global__ __launch_bounds__(CULL_T) void k_cull_compact_copy(int npoints, const int32_t* __restrict__ obsStart, const int32_t* __restrict__ obsFrame,
                                                              const int32_t* __restrict__ obsIdx, int nobs, const uint8_t* __restrict__ live,
                                                              const int32_t* __restrict__ refObs, const int32_t* __restrict__ startOut,
                                                              int32_t* __restrict__ frameOut, int32_t* __restrict__ idxOut, int32_t* __restrict__ refOut)
{
    const int p = blockIdx.x * CULL_T + threadIdx.x;
    if (p >= npoints) return;
    const int a = obsStart[p], b = obsStart[p + 1], ref = refObs[p];
    const int w0 = startOut[p];
    int w = w0, refNew = -1;
    if (a >= 0 && b >= a && b <= nobs)
        for (int o = a; o < b; o++) {
            if (!live[o]) continue;
            if (w >= 0 && w < nobs) { frameOut[w] = obsFrame[o]; idxOut[w] = obsIdx[o]; }   // lists that overlap can sum past nobs
            if (o - a == ref) refNew = w - w0;
            w++;
        }
    refOut[p] = refNew;
}

extern "C" {

int pgorb_compact_observations_device(pgorb_ctx* c, int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
                                      const uint8_t* d_obs_live, const int32_t* d_ref_obs, int32_t* d_obs_start_out, int32_t* d_obs_frame_out,
                                      int32_t* d_obs_idx_out, int32_t* d_ref_obs_out, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (npoints < 0 || nobs < 0 || !d_info || !d_obs_start_out || (npoints && (!d_obs_start || !d_ref_obs || !d_ref_obs_out)) ||
        (nobs && (!d_obs_frame || !d_obs_idx || !d_obs_live || !d_obs_frame_out || !d_obs_idx_out)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_compact_observations_device");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cull_compact_scan, dim3(1), dim3(CULL_T), 0, s, npoints, d_obs_start, nobs, d_obs_live, d_obs_start_out, d_info);
    if (npoints)
        hipLaunchKernelGGL(k_cull_compact_copy, dim3((unsigned)((npoints + CULL_T - 1) / CULL_T)), dim3(CULL_T), 0, s, npoints, d_obs_start, d_obs_frame,
                           d_obs_idx, nobs, d_obs_live, d_ref_obs, d_obs_start_out, d_obs_frame_out, d_obs_idx_out, d_ref_obs_out);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cull_compact_scan / k_cull_compact_copy launch failed");
    return 0;
}

int pgorb_map_point_culling_device(pgorb_ctx* c, int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap, int npoints, uint8_t* d_point_bad,
                                   const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs, uint8_t* d_obs_live,
                                   const int32_t* d_first_kf_id, const int32_t* d_visible, const int32_t* d_found, int nrecent, const int32_t* d_recent,
                                   int cur_kf_id, int th_obs, int32_t* d_action, int32_t* d_recent_out, int32_t* d_nrecent_out, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || nrecent < 0 || !d_info || !d_nrecent_out || (nframes && (!d_kf_point || !d_n)) ||
        (npoints && (!d_point_bad || !d_obs_start || !d_first_kf_id || !d_visible || !d_found)) || (nobs && (!d_obs_frame || !d_obs_idx || !d_obs_live)) ||
        (nrecent && (!d_recent || !d_action || !d_recent_out)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_point_culling_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const PgCullTable T = {d_kf_point, d_n, nframes, cap, npoints, d_point_bad, d_obs_start, d_obs_frame, d_obs_idx, nobs, d_obs_live};
    hipLaunchKernelGGL(k_cull_points, dim3(1), dim3(CULL_T), 0, (hipStream_t)stream, T, d_first_kf_id, d_visible, d_found, nrecent, d_recent, cur_kf_id,
                       th_obs, d_action, d_recent_out, d_nrecent_out, d_info);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cull_points launch failed");
    return 0;
}

int pgorb_keyframe_culling_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap,
                                  int npoints, uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx,
                                  int nobs, uint8_t* d_obs_live, int32_t* d_ref_obs, const int32_t* d_kf_order, const uint8_t* d_kf_id0,
                                  const uint8_t* d_kf_not_erase, uint8_t* d_kf_bad, uint8_t* d_kf_to_be_erased, int cur_kf,
                                  int conn_cap, int32_t* d_conn_kf, int32_t* d_conn_w, int32_t* d_nconn, int32_t* d_ord_kf, int32_t* d_ord_w,
                                  int32_t* d_nord, int32_t* d_parent, int list_cap, int32_t* d_record, int32_t* d_row_status, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || conn_cap < 1 || list_cap < 0 || !d_info || (list_cap && !d_record) ||
        (nframes && (!d_kps || !d_kf_point || !d_n || !d_kf_bad || !d_conn_kf || !d_conn_w || !d_nconn || !d_ord_kf || !d_ord_w || !d_nord || !d_parent ||
                     !d_row_status)) ||
        (npoints && (!d_point_bad || !d_obs_start || !d_ref_obs)) || (nobs && (!d_obs_frame || !d_obs_idx || !d_obs_live)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_keyframe_culling_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const size_t oInv = 0, oClaim = ((size_t)std::max(nframes, 1) * 4 + 63) & ~(size_t)63,
                 oPre = oClaim + (((size_t)std::max(npoints, 1) * 4 + 63) & ~(size_t)63), end = oPre + (size_t)conn_cap * 8;
    void* scr;
    int rc = pg_ctx_scratch(c, end, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    if (hipMemsetAsync(b + oInv, 0xFF, oClaim, s) != hipSuccess || hipMemsetAsync(b + oClaim, 0, oPre - oClaim, s) != hipSuccess)
        return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    const PgCullKf B = {{d_kf_point, d_n, nframes, cap, npoints, d_point_bad, d_obs_start, d_obs_frame, d_obs_idx, nobs, d_obs_live},
                        d_kps, d_ref_obs, d_kf_order, d_kf_id0, d_kf_not_erase, d_kf_bad, d_kf_to_be_erased, cur_kf,
                        conn_cap, d_conn_kf, d_conn_w, d_nconn, d_ord_kf, d_ord_w, d_nord, d_parent, list_cap, d_record, d_row_status, d_info,
                        (int32_t*)(b + oInv), (int32_t*)(b + oClaim), (int32_t*)(b + oPre)};
    if (nframes) hipLaunchKernelGGL(k_cull_eval, dim3((unsigned)std::min(conn_cap, std::max(list_cap, 1))), dim3(CULL_T), 0, s, B);
    hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(CULL_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_cull_eval / k_cull_walk launch failed");
    return pg_ctx_scratch_done(c, s);
}

// ---- the host forms: checked, then one synchronous call of the device form
struct PgCullHostTable {
    int nkf; int32_t* const* kfPoint; const int32_t* n; int npoints; const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx;
};

// the slots and the observation lists as both cullings require them; cap = the widest key frame
static int cull_check_table(const char* fn, const PgCullHostTable& H, const void* pointBad, const void* obsLive, int& cap, std::string& msg)
{
    const std::string f(fn);
    cap = 1;
    if (H.nkf < 0 || H.npoints < 0 || (H.nkf && (!H.kfPoint || !H.n)) || (H.npoints && (!H.obsStart || !pointBad))) { msg = "bad argument to " + f; return PGORB_E_ARG; }
    if (H.nkf > PGORB_COVIS_MAX_KF) { msg = "more than PGORB_COVIS_MAX_KF key frames"; return PGORB_E_LIMIT; }
    for (int k = 0; k < H.nkf; k++) {
        if (H.n[k] < 0 || (H.n[k] && !H.kfPoint[k])) { msg = "bad argument to " + f; return PGORB_E_ARG; }
        if (H.n[k] > 16000) { msg = "more than 16000 keypoints"; return PGORB_E_LIMIT; }
        cap = std::max(cap, H.n[k]);
        for (int s = 0; s < H.n[k]; s++)
            if (H.kfPoint[k][s] < -1 || H.kfPoint[k][s] >= H.npoints) { msg = f + ": a slot names a point out of range"; return PGORB_E_ARG; }
    }
    if (!H.npoints) return 0;
    if (H.obsStart[0] != 0) { msg = f + ": obs_start[0] must be 0"; return PGORB_E_ARG; }
    for (int p = 0; p < H.npoints; p++)
        if (H.obsStart[p + 1] < H.obsStart[p]) { msg = f + ": obs_start decreases"; return PGORB_E_ARG; }
    if (H.obsStart[H.npoints] && (!H.obsFrame || !H.obsIdx || !obsLive)) { msg = "bad argument to " + f; return PGORB_E_ARG; }
    std::vector<int32_t> seen((size_t)std::max(H.nkf, 1), -1);
    for (int p = 0; p < H.npoints; p++)
        for (int o = H.obsStart[p]; o < H.obsStart[p + 1]; o++) {
            const int k = H.obsFrame[o];
            if (k < 0 || k >= H.nkf) { msg = f + ": an observation names a key frame out of range"; return PGORB_E_ARG; }
            if (H.obsIdx[o] < 0 || H.obsIdx[o] >= H.n[k]) { msg = f + ": an observation names a keypoint out of range"; return PGORB_E_ARG; }
            if (seen[k] == p) { msg = f + ": a list names a key frame twice"; return PGORB_E_ARG; }
            seen[k] = p;
        }
    return 0;
}

// the slots as one [nf][cap] block padded with -1, and back
static void cull_pack_slots(int32_t* dst, const PgCullHostTable& H, int nf, int cap)
{
    for (int k = 0; k < nf; k++)
        for (int s = 0; s < cap; s++) dst[(size_t)k * cap + s] = (k < H.nkf && s < H.n[k]) ? H.kfPoint[k][s] : -1;
}
static void cull_unpack_slots(const int32_t* src, const PgCullHostTable& H, int cap)
{
    for (int k = 0; k < H.nkf; k++)
        if (H.n[k]) memcpy(H.kfPoint[k], src + (size_t)k * cap, (size_t)H.n[k] * 4);
}

int pgorb_map_point_culling(pgorb_ctx* c, int nkf, int32_t* const* kf_point, const int32_t* n, int npoints, uint8_t* point_bad,
                            const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx, uint8_t* obs_live,
                            const int32_t* first_kf_id, const int32_t* visible, const int32_t* found, int nrecent, const int32_t* recent,
                            int cur_kf_id, int th_obs, int32_t* action, int32_t* recent_out, int32_t* nrecent_out, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* fn = "pgorb_map_point_culling";
    if (nrecent < 0 || !info || !nrecent_out || (nrecent && (!recent || !action || !recent_out)) || (npoints > 0 && (!first_kf_id || !visible || !found)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_point_culling");
    const PgCullHostTable H = {nkf, kf_point, n, npoints, obs_start, obs_frame, obs_idx};
    std::string msg;
    int cap, rc = cull_check_table(fn, H, point_bad, obs_live, cap, msg);
    if (rc) return pg_ctx_fail(c, rc, msg.c_str());
    {
        std::vector<uint8_t> seen((size_t)std::max(npoints, 1), 0);
        for (int t = 0; t < nrecent; t++) {
            if (recent[t] < 0 || recent[t] >= npoints) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_map_point_culling: a recent entry is out of range");
            if (seen[recent[t]]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_map_point_culling: the recent list names a point twice");
            seen[recent[t]] = 1;
        }
    }
    const int nf = std::max(nkf, 1), np = std::max(npoints, 1), nobs = npoints ? obs_start[npoints] : 0, no = std::max(nobs, 1), nr = std::max(nrecent, 1);
    PgHostCall hc(c);
    const size_t oN = hc.region(PG_UP, (size_t)nf * 4), oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = hc.region(PG_UP, (size_t)no * 4),
                 oOI = hc.region(PG_UP, (size_t)no * 4), oFi = hc.region(PG_UP, (size_t)np * 4), oVi = hc.region(PG_UP, (size_t)np * 4),
                 oFo = hc.region(PG_UP, (size_t)np * 4), oR = hc.region(PG_UP, (size_t)nr * 4),
                 oS = hc.region(PG_INOUT, (size_t)nf * cap * 4), oB = hc.region(PG_INOUT, np), oL = hc.region(PG_INOUT, no),
                 oRO = hc.region(PG_INOUT, (size_t)nr * 4), oA = hc.region(PG_DOWN, (size_t)nr * 4), oOut = hc.region(PG_DOWN, 32);
    if ((rc = hc.begin())) return rc;
    cull_pack_slots(hc.host<int32_t>(oS), H, nf, cap);
    hc.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    if (npoints) hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4); else hc.put(oOS, nullptr, 0, 0, 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oFi, first_kf_id, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oVi, visible, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oFo, found, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oR, recent, (size_t)nrecent * 4, 0, (size_t)nr * 4);
    hc.put(oB, point_bad, npoints, 0, np);
    hc.put(oL, obs_live, nobs, 0, no);
    hc.put(oRO, recent_out, (size_t)nrecent * 4, 0, (size_t)nr * 4);
    if ((rc = hc.run([&] {
            return pgorb_map_point_culling_device(c, hc.dev<int32_t>(oS), hc.dev<int32_t>(oN), nkf, cap, npoints, hc.dev(oB), hc.dev<int32_t>(oOS),
                                                  hc.dev<int32_t>(oOF), hc.dev<int32_t>(oOI), nobs, hc.dev(oL), hc.dev<int32_t>(oFi), hc.dev<int32_t>(oVi),
                                                  hc.dev<int32_t>(oFo), nrecent, hc.dev<int32_t>(oR), cur_kf_id, th_obs, hc.dev<int32_t>(oA),
                                                  hc.dev<int32_t>(oRO), hc.dev<int32_t>(oOut), hc.dev<int32_t>(oOut) + 4, nullptr); }))) return rc;
    cull_unpack_slots(hc.host<int32_t>(oS), H, cap);
    if (npoints) memcpy(point_bad, hc.host(oB), npoints);
    if (nobs) memcpy(obs_live, hc.host(oL), nobs);
    if (nrecent) { memcpy(recent_out, hc.host(oRO), (size_t)nrecent * 4); memcpy(action, hc.host(oA), (size_t)nrecent * 4); }
    *nrecent_out = hc.host<int32_t>(oOut)[0];
    memcpy(info, hc.host<int32_t>(oOut) + 4, PGORB_CULL_INFO * 4);
    return info[2];
}

int pgorb_keyframe_culling(pgorb_ctx* c, int nkf, const pgorb_keypoint* const* kps, int32_t* const* kf_point, const int32_t* n,
                           int npoints, uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx,
                           uint8_t* obs_live, int32_t* ref_obs, const int32_t* kf_order, const uint8_t* kf_id0, const uint8_t* kf_not_erase,
                           uint8_t* kf_bad, uint8_t* kf_to_be_erased, int cur_kf, int conn_cap, int32_t* conn_kf, int32_t* conn_w, int32_t* nconn,
                           int32_t* ord_kf, int32_t* ord_w, int32_t* nord, int32_t* parent, int list_cap, int32_t* record, int32_t* row_status, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* fn = "pgorb_keyframe_culling";
    const char* bad = "bad argument to pgorb_keyframe_culling";
    if (conn_cap < 1 || list_cap < 1 || !record || !info || cur_kf < 0 || cur_kf >= nkf || (npoints > 0 && !ref_obs) ||
        (nkf > 0 && (!kps || !kf_bad || !conn_kf || !conn_w || !nconn || !ord_kf || !ord_w || !nord || !parent || !row_status)))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (conn_cap > PGORB_COVIS_MAX_CONN) return pg_ctx_fail(c, PGORB_E_LIMIT, "conn_cap above PGORB_COVIS_MAX_CONN");
    const PgCullHostTable H = {nkf, kf_point, n, npoints, obs_start, obs_frame, obs_idx};
    std::string msg;
    int cap, rc = cull_check_table(fn, H, point_bad, obs_live, cap, msg);
    if (rc) return pg_ctx_fail(c, rc, msg.c_str());
    for (int k = 0; k < nkf; k++)
        if (n[k] && !kps[k]) return pg_ctx_fail(c, PGORB_E_ARG, bad);
    for (int p = 0; p < npoints; p++) {
        const int len = obs_start[p + 1] - obs_start[p];
        if (len && (ref_obs[p] < -1 || ref_obs[p] >= len)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: ref_obs is outside its list");
    }
    {
        std::vector<int32_t> mark((size_t)nkf, -1);
        if (kf_order) {
            for (int k = 0; k < nkf; k++) {
                if (kf_order[k] < 0 || kf_order[k] >= nkf || mark[kf_order[k]] >= 0) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: kf_order is not a permutation");
                mark[kf_order[k]] = k;
            }
            std::fill(mark.begin(), mark.end(), -1);
        }
        for (int k = 0; k < nkf; k++) {
            if (nconn[k] < 0 || nconn[k] > conn_cap || nord[k] < 0 || nord[k] > conn_cap)
                return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: a row count is outside [0, conn_cap]");
            if (parent[k] < -1 || parent[k] >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: a parent is out of range");
            int last = -1;
            for (int t = 0; t < nconn[k]; t++) {
                const int j = conn_kf[(size_t)k * conn_cap + t];
                if (j < 0 || j >= nkf || j == k) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: a connection is out of range");
                const int r = kf_order ? kf_order[j] : j;
                if (r <= last) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: a connection row is not in address order");
                last = r;
                mark[j] = k;
            }
            for (int t = 0; t < nord[k]; t++) {
                const int j = ord_kf[(size_t)k * conn_cap + t];
                if (j < 0 || j >= nkf || mark[j] != k) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_keyframe_culling: an ordered entry is not in the row's map");
            }
        }
    }
    const int np = std::max(npoints, 1), nobs = npoints ? obs_start[npoints] : 0, no = std::max(nobs, 1);
    const size_t rowB = (size_t)nkf * conn_cap * 4, kpB = (size_t)nkf * cap * sizeof(pgorb_keypoint);
    PgHostCall hc(c);
    const size_t oK = hc.region(PG_UP, kpB), oN = hc.region(PG_UP, (size_t)nkf * 4), oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4),
                 oOF = hc.region(PG_UP, (size_t)no * 4), oOI = hc.region(PG_UP, (size_t)no * 4), oOrd = hc.region(PG_UP, (size_t)nkf * 4),
                 oId0 = hc.region(PG_UP, nkf), oNE = hc.region(PG_UP, nkf),
                 oS = hc.region(PG_INOUT, (size_t)nkf * cap * 4), oB = hc.region(PG_INOUT, np), oL = hc.region(PG_INOUT, no),
                 oRef = hc.region(PG_INOUT, (size_t)np * 4), oKB = hc.region(PG_INOUT, nkf), oTBE = hc.region(PG_INOUT, nkf),
                 oCK = hc.region(PG_INOUT, rowB), oCW = hc.region(PG_INOUT, rowB), oNC = hc.region(PG_INOUT, (size_t)nkf * 4),
                 oOK = hc.region(PG_INOUT, rowB), oOW = hc.region(PG_INOUT, rowB), oNO = hc.region(PG_INOUT, (size_t)nkf * 4),
                 oPar = hc.region(PG_INOUT, (size_t)nkf * 4), oRec = hc.region(PG_INOUT, (size_t)list_cap * 16),
                 oSt = hc.region(PG_INOUT, (size_t)nkf * 4), oInfo = hc.region(PG_DOWN, PGORB_CULL_INFO * 4);
    if ((rc = hc.begin())) return rc;
    memset(hc.host(oK), 0, kpB);
    for (int k = 0; k < nkf; k++)
        if (n[k]) memcpy(hc.host<pgorb_keypoint>(oK) + (size_t)k * cap, kps[k], (size_t)n[k] * sizeof(pgorb_keypoint));
    cull_pack_slots(hc.host<int32_t>(oS), H, nkf, cap);
    hc.put(oN, n, (size_t)nkf * 4);
    if (npoints) hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4); else hc.put(oOS, nullptr, 0, 0, 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOrd, kf_order, (size_t)nkf * 4, 0, (size_t)nkf * 4);
    hc.put(oId0, kf_id0, nkf, 0, nkf);
    hc.put(oNE, kf_not_erase, nkf, 0, nkf);
    hc.put(oB, point_bad, npoints, 0, np);
    hc.put(oL, obs_live, nobs, 0, no);
    hc.put(oRef, ref_obs, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oKB, kf_bad, nkf);
    hc.put(oTBE, kf_to_be_erased, nkf, 0, nkf);
    hc.put(oCK, conn_kf, rowB); hc.put(oCW, conn_w, rowB); hc.put(oNC, nconn, (size_t)nkf * 4);
    hc.put(oOK, ord_kf, rowB); hc.put(oOW, ord_w, rowB); hc.put(oNO, nord, (size_t)nkf * 4);
    hc.put(oPar, parent, (size_t)nkf * 4);
    hc.put(oRec, record, (size_t)list_cap * 16);
    hc.put(oSt, row_status, (size_t)nkf * 4);
    if ((rc = hc.run([&] {
            return pgorb_keyframe_culling_device(c, hc.dev<pgorb_keypoint>(oK), hc.dev<int32_t>(oS), hc.dev<int32_t>(oN), nkf, cap, npoints, hc.dev(oB),
                                                 hc.dev<int32_t>(oOS), hc.dev<int32_t>(oOF), hc.dev<int32_t>(oOI), nobs, hc.dev(oL), hc.dev<int32_t>(oRef),
                                                 kf_order ? hc.dev<int32_t>(oOrd) : nullptr, hc.dev(oId0), hc.dev(oNE), hc.dev(oKB), hc.dev(oTBE), cur_kf,
                                                 conn_cap, hc.dev<int32_t>(oCK), hc.dev<int32_t>(oCW), hc.dev<int32_t>(oNC), hc.dev<int32_t>(oOK),
                                                 hc.dev<int32_t>(oOW), hc.dev<int32_t>(oNO), hc.dev<int32_t>(oPar), list_cap, hc.dev<int32_t>(oRec),
                                                 hc.dev<int32_t>(oSt), hc.dev<int32_t>(oInfo), nullptr); }))) return rc;
    cull_unpack_slots(hc.host<int32_t>(oS), H, cap);
    if (npoints) { memcpy(point_bad, hc.host(oB), npoints); memcpy(ref_obs, hc.host(oRef), (size_t)npoints * 4); }
    if (nobs) memcpy(obs_live, hc.host(oL), nobs);
    memcpy(kf_bad, hc.host(oKB), nkf);
    if (kf_to_be_erased) memcpy(kf_to_be_erased, hc.host(oTBE), nkf);
    memcpy(conn_kf, hc.host(oCK), rowB); memcpy(conn_w, hc.host(oCW), rowB); memcpy(nconn, hc.host(oNC), (size_t)nkf * 4);
    memcpy(ord_kf, hc.host(oOK), rowB); memcpy(ord_w, hc.host(oOW), rowB); memcpy(nord, hc.host(oNO), (size_t)nkf * 4);
    memcpy(parent, hc.host(oPar), (size_t)nkf * 4);
    memcpy(record, hc.host(oRec), (size_t)list_cap * 16);
    memcpy(row_status, hc.host(oSt), (size_t)nkf * 4);
    memcpy(info, hc.host(oInfo), PGORB_CULL_INFO * 4);
    return info[2];
}

}  // extern "C"
