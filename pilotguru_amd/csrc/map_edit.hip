// map_edit.hip -- the map's three mutators and their key-frame slot writes, run on the device from an ordered edit list, next to the
// cullings, on gfx950.  Integers only, every result exact and a function of the inputs alone.
//
// Restates (thirdparty/orb-slam2):
//   MapPoint::AddObservation, EraseObservation     src/MapPoint.cc:119-130, :132-158
//   MapPoint::SetBadFlag, Replace                  src/MapPoint.cc:172-187, :196-232
//   KeyFrame::AddMapPoint, EraseMapPointMatch      src/KeyFrame.cc:313-336
//
// No edit reads a slot: the mutators read and write per-point state and only WRITE slots.  So the points that REPLACE edits link
// form components whose edits are a subsequence of the list, components share no per-point state, and a slot ends as the value
// of the last edit in list order that writes it.
//   k_edit_init         a thread per point: the working copy of the per-point state, the live length of every list
//   k_edit_components   ONE workgroup: the components by min-hooking over the REPLACE pairs until nothing changes
//   k_edit_bucket       ONE workgroup: the edits that are carried out (not NOP, in range) counted and numbered in list order, at most
//                       PGORB_EDIT_MAX_EDITS of them sorted by (component, list position) in LDS, the component table
//   k_edit_plan         a wave per component walks its edits in order over one flat bag of (point, key frame, keypoint) in LDS;
//                       a REPLACE relabels the loser's entries or kills them.  It writes scratch only: the new lists sorted by
//                       (point, address rank), the last write per slot, the per-point state, the edit status
//   k_edit_scan         ONE workgroup: the new obs_start, the selection, the counts -- and the limit decision.  Nothing before
//                       it writes an in/out or output byte
//   k_edit_mark         a thread per slot record: atomicMax of (marker | edit index) into the slot -- the last writer's mark,
//                       whatever the order of the atomics
//   k_edit_commit       the record that finds its own mark writes its value; a thread per point writes the lists, ref_obs, the
//                       flags and counters; a thread per edit its status.  Both skipped under the limit flag.
#include "match_common.h"
#include <string>
#include <vector>

#define EDIT_T 256
#define EDIT_CT 1024                     // k_edit_components / k_edit_bucket
#define EDIT_MARK 0x40000000             // above every point index (npoints <= 2^30)

enum { EC_LIMIT, EC_NCOMP, EC_ENTRIES, EC_RECORDS, EC_APPLIED, EC_WRITES, EC_COUNT = 16 };

struct PgEdit {
    const pgorb_map_edit* edits; int nedits; const int32_t* nedPtr;
    int32_t* kfPoint; const int32_t* n; int nframes; int cap; const int32_t* order;
    int npoints; uint8_t* pbad; int32_t* visible; int32_t* found; int32_t* replaced;
    const int32_t* obsStart; const int32_t* obsFrame; const int32_t* obsIdx; int nobs; const uint8_t* live; const int32_t* refObs;
    int obsCapOut; int32_t* startOut; int32_t* frameOut; int32_t* idxOut; int32_t* refOut;
    int32_t* statusOut; int32_t* touchedOut; int selectBits; int selCap; int32_t* selectOut; int32_t* info;
    // scratch: per point
    int32_t* comp; int32_t* sBad; int32_t* sVis; int32_t* sFound; int32_t* sRepl; int32_t* sRef; int32_t* sTouched; int32_t* newLen;
    int32_t* outPos; int32_t* loaded;
    // per edit
    int32_t* sorted; int32_t* compFirst; int32_t* status;
    // pools of ecap = nobs + nedits
    int ecap; int32_t* eKf; int32_t* eIdx; int32_t* rSlot; int32_t* rVal; int32_t* rEd;
    int32_t* cnt;
};

__device__ __forceinline__ int edit_count(const PgEdit& B)
{
    return B.nedPtr ? min(max(B.nedPtr[0], 0), B.nedits) : B.nedits;
}

// the list of point p as [x, y); empty when the pair is no list
__device__ __forceinline__ int2 edit_range(const PgEdit& B, int p)
{
    const int a = B.obsStart[p], b = B.obsStart[p + 1];
    return (a < 0 || b < a || b > B.nobs) ? make_int2(0, 0) : make_int2(a, b);
}

// observation o as (key frame, keypoint): false when it is dead or names nothing of the batch
__device__ __forceinline__ bool edit_obs(const PgEdit& B, int o, int& f, int& i)
{
    if (B.live && !B.live[o]) return false;
    f = B.obsFrame[o]; i = B.obsIdx[o];
    if (f < 0 || f >= B.nframes) return false;
    return i >= 0 && i < min(max(B.n[f], 0), B.cap);
}

__device__ __forceinline__ bool edit_point_ok(const PgEdit& B, int p) { return p >= 0 && p < B.npoints; }
__device__ __forceinline__ bool edit_kf_ok(const PgEdit& B, int f) { return f >= 0 && f < B.nframes; }

// is the edit carried out at all (its indices in range)?  NOP and unknown ops are not
__device__ __forceinline__ bool edit_valid(const PgEdit& B, const pgorb_map_edit& e)
{
    switch (e.op) {
    case PGORB_EDIT_ADD: return edit_point_ok(B, e.a) && edit_kf_ok(B, e.b) && e.c >= 0 && e.c < min(max(B.n[e.b], 0), B.cap);
    case PGORB_EDIT_REPLACE: return edit_point_ok(B, e.a) && edit_point_ok(B, e.b);
    case PGORB_EDIT_ERASE:
    case PGORB_EDIT_SET_REF: return edit_point_ok(B, e.a) && edit_kf_ok(B, e.b);
    }
    return false;
}

__device__ __forceinline__ int edit_rank(const PgEdit& B, int f) { return (B.order ? B.order[f] : f) & 0x1FFF; }

__device__ __forceinline__ int edit_find_root(const int32_t* comp, int x)
{
    for (;;) {
        const int c = __atomic_load_n(&comp[x], __ATOMIC_RELAXED);                 // comp[x] <= x, the chain only descends
        if (c == x) return x;
        x = c;
    }
}

__global__ __launch_bounds__(EDIT_T) void k_edit_init(PgEdit B)
{
    const int p = blockIdx.x * EDIT_T + threadIdx.x;
    if (p >= B.npoints) return;
    const int2 r = edit_range(B, p);
    int cnt = 0, f, i;
    for (int o = r.x; o < r.y; o++) cnt += edit_obs(B, o, f, i);
    const int ro = B.refObs[p];
    int ref = -1;
    if (ro >= 0 && ro < r.y - r.x && edit_obs(B, r.x + ro, f, i)) ref = f;         // mpRefKF by key frame; a dead entry names none
    B.comp[p] = p;
    B.sBad[p] = B.pbad[p] != 0;
    B.sVis[p] = B.visible ? B.visible[p] : 0;
    B.sFound[p] = B.found ? B.found[p] : 0;
    B.sRepl[p] = B.replaced ? B.replaced[p] : -1;
    B.sRef[p] = ref;
    B.sTouched[p] = 0;
    B.newLen[p] = cnt;
    B.outPos[p] = 0;
    B.loaded[p] = 0;
}

__global__ __launch_bounds__(EDIT_CT) void k_edit_components(PgEdit B)
{
    __shared__ int sChanged;
    const int ne = edit_count(B);
    for (;;) {
        if (threadIdx.x == 0) sChanged = 0;
        __syncthreads();
        for (int e = threadIdx.x; e < ne; e += EDIT_CT) {
            const pgorb_map_edit ed = B.edits[e];
            if (ed.op != PGORB_EDIT_REPLACE || ed.a == ed.b || !edit_valid(B, ed)) continue;
            const int ra = edit_find_root(B.comp, ed.a), rb = edit_find_root(B.comp, ed.b);
            if (ra == rb) continue;
            atomicMin(&B.comp[max(ra, rb)], min(ra, rb));                          // a lost hook is made again in the next round
            sChanged = 1;
        }
        __threadfence_block();
        __syncthreads();
        if (!sChanged) break;                                                      // a round without a hook: every pair shares its root
        __syncthreads();
    }
}

// ascending bitonic sort of key[0 .. m), m a power of two, by the whole workgroup of T threads
template <int T> __device__ __forceinline__ void edit_sort(unsigned long long* key, int m)
{
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < m; t += T) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long a = key[t], b = key[x];
                    if (((t & k) == 0) ? (a > b) : (a < b)) { key[t] = b; key[x] = a; }
                }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(EDIT_CT) void k_edit_bucket(PgEdit B)
{
    __shared__ unsigned long long key[PGORB_EDIT_MAX_EDITS];
    __shared__ int part[EDIT_CT + 1];
    const int tid = threadIdx.x, ne = edit_count(B);
    // the edits that are carried out, counted and then numbered in list order: a thread takes a run of the list
    const int run = (ne + EDIT_CT - 1) / EDIT_CT, e0 = min(tid * run, ne), e1 = min(e0 + run, ne);
    int mine = 0;
    for (int e = e0; e < e1; e++) {
        const pgorb_map_edit ed = B.edits[e];
        if (ed.op == PGORB_EDIT_NOP) continue;
        if (edit_valid(B, ed)) mine++;
        else B.status[e] = PGORB_EDIT_BAD_INDEX;
    }
    part[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int k = 0; k < EDIT_CT; k++) { const int v = part[k]; part[k] = sum; sum += v; }
        part[EDIT_CT] = sum;
    }
    __syncthreads();
    const int nv = part[EDIT_CT];
    if (nv > PGORB_EDIT_MAX_EDITS) {                                               // more than the sort holds: the scan reports the limit, nothing is planned
        if (tid == 0) { B.cnt[EC_LIMIT] = 1; B.cnt[EC_NCOMP] = 0; }
        return;
    }
    int m2 = 1;
    while (m2 < nv) m2 <<= 1;
    int at = part[tid];
    for (int e = e0; e < e1; e++) {
        const pgorb_map_edit ed = B.edits[e];
        if (ed.op != PGORB_EDIT_NOP && edit_valid(B, ed)) key[at++] = ((unsigned long long)(unsigned)edit_find_root(B.comp, ed.a) << 32) | (unsigned)e;
    }
    for (int t = nv + tid; t < m2; t += EDIT_CT) key[t] = ~0ull;
    __syncthreads();                                                               // part is read above and written below
    edit_sort<EDIT_CT>(key, m2);
    const int chunk = (m2 + EDIT_CT - 1) / EDIT_CT, t0 = min(tid * chunk, nv), t1 = min(t0 + chunk, nv);
    int heads = 0;
    for (int t = t0; t < t1; t++) heads += t == 0 || (key[t] >> 32) != (key[t - 1] >> 32);
    part[tid] = heads;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int k = 0; k < EDIT_CT; k++) { const int v = part[k]; part[k] = sum; sum += v; }
        part[EDIT_CT] = sum;
    }
    __syncthreads();
    int ci = part[tid];
    for (int t = t0; t < t1; t++) {
        B.sorted[t] = (int)(unsigned)(key[t] & 0xFFFFFFFFu);
        if (t == 0 || (key[t] >> 32) != (key[t - 1] >> 32)) B.compFirst[ci++] = t;
    }
    if (tid == 0) { B.compFirst[part[EDIT_CT]] = nv; B.cnt[EC_NCOMP] = part[EDIT_CT]; }
}

// ---- the plan: one wave, one component
struct PgEditBag {
    int32_t* pt; int32_t* kf; int32_t* idx;                                        // the observations of the component; pt < 0 = killed
    int32_t* pSlot; int32_t* pVal; int32_t* pEd;                                   // the last write per slot so far
    int* hit;
    int nb, np, used;                                                              // wave-uniform: entries, pending slots, entries + ADD edits
};

// the live list of p joins the bag the first time an edit names p
__device__ void edit_load(const PgEdit& B, PgEditBag& S, int p)
{
    if (B.loaded[p]) return;
    const int lane = threadIdx.x;
    const int2 r = edit_range(B, p);
    for (int o0 = r.x; o0 < r.y; o0 += 64) {
        const int o = o0 + lane;
        int f = 0, i = 0;
        const bool ok = o < r.y && edit_obs(B, o, f, i);
        const unsigned long long m = __ballot(ok);
        const int at = S.nb + __popcll(m & ((1ull << lane) - 1));
        if (ok && at < PGORB_EDIT_MAX_BAG) { S.pt[at] = p; S.kf[at] = f; S.idx[at] = i; }
        S.nb += __popcll(m); S.used += __popcll(m);
    }
    if (lane == 0) { B.loaded[p] = 1; B.newLen[p] = 0; }
    __threadfence_block();
    __syncthreads();
}

// the entry (p, f), or any entry of p when f < 0; -1 = none.  A list holds a key frame once, so at most one lane finds it
__device__ int edit_find(PgEditBag& S, int p, int f)
{
    const int lane = threadIdx.x;
    if (lane == 0) *S.hit = -1;
    __syncthreads();
    for (int t = lane; t < S.nb; t += 64)
        if (S.pt[t] == p && (f < 0 || S.kf[t] == f)) atomicMax(S.hit, t);
    __syncthreads();
    const int h = *S.hit;
    __syncthreads();
    return h;
}

// one slot write of edit e: it takes the place of an earlier write to the same slot
__device__ void edit_slot(PgEditBag& S, int slot, int val, int e)
{
    const int lane = threadIdx.x;
    if (lane == 0) *S.hit = -1;
    __syncthreads();
    for (int t = lane; t < S.np; t += 64)
        if (S.pSlot[t] == slot) *S.hit = t;
    __syncthreads();
    const int h = *S.hit;
    const int at = h >= 0 ? h : S.np;
    if (lane == 0 && at < PGORB_EDIT_MAX_BAG) { S.pSlot[at] = slot; S.pVal[at] = val; S.pEd[at] = e; }
    if (h < 0) S.np++;
    __syncthreads();
}

// p's list changed: a change after its last REPLACE as the survivor leaves the reference's descriptor older than the list
__device__ __forceinline__ void edit_changed(const PgEdit& B, int p)
{
    const int t = B.sTouched[p];
    B.sTouched[p] = t | PGORB_EDIT_TOUCH_CHANGED | ((t & PGORB_EDIT_TOUCH_SURVIVOR) ? PGORB_EDIT_TOUCH_STALE : 0);
}

__global__ __launch_bounds__(64) void k_edit_plan(PgEdit B)
{
    __shared__ int32_t sPt[PGORB_EDIT_MAX_BAG], sKf[PGORB_EDIT_MAX_BAG], sIdx[PGORB_EDIT_MAX_BAG];
    __shared__ unsigned long long sKey[PGORB_EDIT_MAX_BAG * 3 / 2];                 // the pending slot writes; afterwards the sort keys
    __shared__ int sHit, sCnt, sBest, sBase;
    const int lane = threadIdx.x, ci = blockIdx.x;
    if (ci >= B.cnt[EC_NCOMP]) return;
    const int first = B.compFirst[ci], nc = B.compFirst[ci + 1] - first;
    PgEditBag S = {sPt, sKf, sIdx, (int32_t*)sKey, (int32_t*)sKey + PGORB_EDIT_MAX_BAG, (int32_t*)sKey + 2 * PGORB_EDIT_MAX_BAG, &sHit, 0, 0, 0};
    int applied = 0, writes = 0;
    bool over = false;
    for (int k = 0; k < nc && !over; k++) {
        const int e = B.sorted[first + k];
        const pgorb_map_edit ed = B.edits[e];
        const int a = ed.a, b = ed.b;
        int st = PGORB_EDIT_APPLIED;
        if (ed.op == PGORB_EDIT_ADD) {                                             // AddObservation, then AddMapPoint whatever it did
            edit_load(B, S, a);
            S.used++;
            if ((over = S.used > PGORB_EDIT_MAX_BAG)) break;
            if (edit_find(S, a, b) < 0) {
                if (lane == 0) { sPt[S.nb] = a; sKf[S.nb] = b; sIdx[S.nb] = ed.c; edit_changed(B, a); }
                S.nb++;
            } else st |= PGORB_EDIT_ALREADY;
            edit_slot(S, b * B.cap + ed.c, a, e);
            writes++;
        } else if (ed.op == PGORB_EDIT_REPLACE) {
            if (a == b) st = PGORB_EDIT_SELF;
            else {
                edit_load(B, S, a);
                edit_load(B, S, b);
                if ((over = S.used > PGORB_EDIT_MAX_BAG)) break;
                int len = 0, gained = 0;
                for (int t0 = 0; t0 < S.nb; t0 += 64) {
                    const int t = t0 + lane;
                    const bool mine = t < S.nb && sPt[t] == a;
                    bool has = false;
                    int hit = -1, slot = 0;
                    if (mine) {
                        const int f = sKf[t];
                        for (int j = 0; j < S.nb && !has; j++) has = sPt[j] == b && sKf[j] == f;
                        slot = f * B.cap + sIdx[t];
                        for (int j = 0; j < S.np && hit < 0; j++)
                            if (S.pSlot[j] == slot) hit = j;
                    }
                    __syncthreads();
                    const unsigned long long mApp = __ballot(mine && hit < 0);
                    const int at = hit >= 0 ? hit : S.np + __popcll(mApp & ((1ull << lane) - 1));
                    if (mine) {
                        if (at < PGORB_EDIT_MAX_BAG) { S.pSlot[at] = slot; S.pVal[at] = has ? -1 : b; S.pEd[at] = e; }
                        sPt[t] = has ? -1 : b;                                     // joins the survivor, or leaves the map
                    }
                    S.np += __popcll(mApp);
                    len += __popcll(__ballot(mine));
                    gained += __popcll(__ballot(mine && !has));
                    __syncthreads();
                }
                writes += len;
                if (lane == 0) {
                    if (len) B.sTouched[a] |= PGORB_EDIT_TOUCH_CHANGED;
                    B.sBad[a] = 1; B.sRepl[a] = b;
                    B.sFound[b] = (int)((unsigned)B.sFound[b] + (unsigned)B.sFound[a]);
                    B.sVis[b] = (int)((unsigned)B.sVis[b] + (unsigned)B.sVis[a]);
                    if (gained) B.sTouched[b] |= PGORB_EDIT_TOUCH_CHANGED;
                    B.sTouched[b] = (B.sTouched[b] | PGORB_EDIT_TOUCH_SURVIVOR) & ~PGORB_EDIT_TOUCH_STALE;   // the descriptor due is computed after this edit
                }
            }
        } else if (ed.op == PGORB_EDIT_ERASE) {                                    // EraseMapPointMatch(MapPoint*), then EraseObservation
            edit_load(B, S, a);
            if ((over = S.used > PGORB_EDIT_MAX_BAG)) break;
            const int h = edit_find(S, a, b);
            if (h < 0) st = PGORB_EDIT_NOT_OBSERVED;
            else {
                edit_slot(S, b * B.cap + sIdx[h], -1, e);
                writes++;
                if (lane == 0) { sPt[h] = -1; sCnt = 0; sBest = 0x7FFFFFFF; edit_changed(B, a); }
                __syncthreads();
                for (int t = lane; t < S.nb; t += 64)
                    if (sPt[t] == a) { atomicAdd(&sCnt, 1); atomicMin(&sBest, (edit_rank(B, sKf[t]) << 13) | sKf[t]); }
                __syncthreads();
                const int left = sCnt, best = sBest;
                __syncthreads();
                if (lane == 0 && B.sRef[a] == b) B.sRef[a] = left ? (best & 0x1FFF) : -1;   // begin() of what is left; of nothing: none
                if (left <= 2) {                                                   // SetBadFlag: every remaining slot cleared, mpRefKF kept
                    st |= PGORB_EDIT_WENT_BAD;
                    if (lane == 0) B.sBad[a] = 1;
                    for (int q = 0; q < left; q++) {
                        const int h2 = edit_find(S, a, -1);
                        if (h2 < 0) break;
                        edit_slot(S, sKf[h2] * B.cap + sIdx[h2], -1, e);
                        writes++;
                        if (lane == 0) sPt[h2] = -1;
                        __syncthreads();
                    }
                }
            }
        } else if (lane == 0) B.sRef[a] = b;                                       // PGORB_EDIT_SET_REF
        if (lane == 0) B.status[e] = st;
        applied += (st & PGORB_EDIT_APPLIED) != 0;
        __threadfence_block();
        __syncthreads();
    }
    if (over) { if (lane == 0) B.cnt[EC_LIMIT] = 1; return; }
    // the last write per slot leaves for the record pool
    if (lane == 0) sBase = atomicAdd(&B.cnt[EC_RECORDS], S.np);                     // where in the pool reaches no output: the commit goes by (slot, edit)
    __syncthreads();
    const int rbase = sBase;
    __syncthreads();
    if (rbase + S.np > B.ecap) { if (lane == 0) B.cnt[EC_LIMIT] = 1; return; }
    for (int t = lane; t < S.np; t += 64) { B.rSlot[rbase + t] = S.pSlot[t]; B.rVal[rbase + t] = S.pVal[t]; B.rEd[rbase + t] = S.pEd[t]; }
    __syncthreads();
    // the lists that are left, sorted by (point, address rank)
    int nlive = 0;
    for (int t0 = 0; t0 < S.nb; t0 += 64) {
        const int t = t0 + lane;
        const bool ok = t < S.nb && sPt[t] >= 0;
        const unsigned long long m = __ballot(ok);
        if (ok) sKey[nlive + __popcll(m & ((1ull << lane) - 1))] = ((unsigned long long)(unsigned)sPt[t] << 24) | ((unsigned long long)edit_rank(B, sKf[t]) << 11) | (unsigned)t;
        nlive += __popcll(m);
    }
    int m2 = 1;
    while (m2 < nlive) m2 <<= 1;
    for (int t = nlive + lane; t < m2; t += 64) sKey[t] = ~0ull;
    edit_sort<64>(sKey, m2);
    if (lane == 0) sBase = atomicAdd(&B.cnt[EC_ENTRIES], nlive);
    __syncthreads();
    const int ebase = sBase;
    if (ebase + nlive > B.ecap) { if (lane == 0) B.cnt[EC_LIMIT] = 1; return; }
    for (int t = lane; t < nlive; t += 64) {
        const int src = (int)(sKey[t] & 0x7FF), p = (int)(sKey[t] >> 24);
        B.eKf[ebase + t] = sKf[src]; B.eIdx[ebase + t] = sIdx[src];
        if (t == 0 || (int)(sKey[t - 1] >> 24) != p) {
            int len = 1;
            while (t + len < nlive && (int)(sKey[t + len] >> 24) == p) len++;
            B.newLen[p] = len; B.outPos[p] = ebase + t;
        }
    }
    if (lane == 0) { atomicAdd(&B.cnt[EC_APPLIED], applied); atomicAdd(&B.cnt[EC_WRITES], writes); }
}

__global__ __launch_bounds__(EDIT_T) void k_edit_scan(PgEdit B)
{
    __shared__ int32_t part[4][EDIT_T + 1];
    __shared__ int sLimit;
    const int t = threadIdx.x, np = B.npoints;
    const bool sel = B.selectOut && B.selCap > 0;
    const int chunk = (np + EDIT_T - 1) / EDIT_T, k0 = min(t * chunk, np), k1 = min(k0 + chunk, np);
    int s[4] = {0, 0, 0, 0};                                                        // entries, selected, went bad, stale
    for (int p = k0; p < k1; p++) {
        s[0] += B.newLen[p];
        s[1] += sel && (B.sTouched[p] & B.selectBits) != 0;
        s[2] += B.sBad[p] && !B.pbad[p];
        s[3] += (B.sTouched[p] & PGORB_EDIT_TOUCH_STALE) != 0;
    }
    for (int q = 0; q < 4; q++) part[q][t] = s[q];
    __syncthreads();
    if (t == 0) {
        for (int q = 0; q < 4; q++) {
            int run = 0;
            for (int k = 0; k < EDIT_T; k++) { const int v = part[q][k]; part[q][k] = run; run += v; }
            part[q][EDIT_T] = run;
        }
        const bool limit = B.cnt[EC_LIMIT] || part[0][EDIT_T] > B.obsCapOut || part[0][EDIT_T] < 0 || part[1][EDIT_T] > B.selCap;
        sLimit = limit;
        B.cnt[EC_LIMIT] = limit;
        B.info[0] = limit ? PGORB_EDIT_LIMIT : 0;
        if (!limit) {
            B.info[1] = part[0][EDIT_T]; B.info[2] = B.cnt[EC_APPLIED]; B.info[3] = part[2][EDIT_T]; B.info[4] = B.cnt[EC_NCOMP];
            B.info[5] = B.cnt[EC_WRITES]; B.info[6] = part[3][EDIT_T]; B.info[7] = part[1][EDIT_T];
            B.startOut[np] = part[0][EDIT_T];
        }
    }
    __syncthreads();
    if (sLimit) return;
    int run = part[0][t], at = part[1][t];
    for (int p = k0; p < k1; p++) {
        B.startOut[p] = run;
        run += B.newLen[p];
        if (sel && (B.sTouched[p] & B.selectBits) != 0) B.selectOut[at++] = p;
    }
    if (sel)
        for (int k = part[1][EDIT_T] + t; k < B.selCap; k += EDIT_T) B.selectOut[k] = -1;
}

__global__ __launch_bounds__(EDIT_T) void k_edit_mark(PgEdit B)
{
    if (B.cnt[EC_LIMIT]) return;
    const int r = blockIdx.x * EDIT_T + threadIdx.x;
    if (r < min(B.cnt[EC_RECORDS], B.ecap)) atomicMax(&B.kfPoint[B.rSlot[r]], EDIT_MARK | B.rEd[r]);
}

__global__ __launch_bounds__(EDIT_T) void k_edit_commit(PgEdit B)
{
    if (B.cnt[EC_LIMIT]) return;
    const int x = blockIdx.x * EDIT_T + threadIdx.x;
    if (x < min(B.cnt[EC_RECORDS], B.ecap) && B.kfPoint[B.rSlot[x]] == (EDIT_MARK | B.rEd[x])) B.kfPoint[B.rSlot[x]] = B.rVal[x];   // (slot, edit) is one record's
    if (x < B.nedits) B.statusOut[x] = x < edit_count(B) ? B.status[x] : 0;
    if (x >= B.npoints) return;
    const int p = x, w0 = B.startOut[p], ref = B.sRef[p];
    int refNew = -1;
    if (B.loaded[p]) {
        const int len = B.newLen[p], src = B.outPos[p];
        for (int k = 0; k < len; k++) {
            const int f = B.eKf[src + k];
            if (w0 + k < B.obsCapOut) { B.frameOut[w0 + k] = f; B.idxOut[w0 + k] = B.eIdx[src + k]; }
            if (f == ref) refNew = k;
        }
    } else {
        const int2 r = edit_range(B, p);
        int w = w0, f, i;
        for (int o = r.x; o < r.y; o++) {
            if (!edit_obs(B, o, f, i)) continue;
            if (w < B.obsCapOut) { B.frameOut[w] = f; B.idxOut[w] = i; }
            if (f == ref) refNew = w - w0;
            w++;
        }
    }
    B.refOut[p] = refNew;
    B.pbad[p] = (uint8_t)(B.sBad[p] != 0);
    if (B.visible) B.visible[p] = B.sVis[p];
    if (B.found) B.found[p] = B.sFound[p];
    if (B.replaced) B.replaced[p] = B.sRepl[p];
    B.touchedOut[p] = B.sTouched[p];
}

static inline size_t edit_al(size_t b) { return (b + 63) & ~(size_t)63; }

extern "C" {

int pgorb_apply_map_edits_device(pgorb_ctx* c, const pgorb_map_edit* d_edits, int nedits, const int32_t* d_nedits, int32_t* d_kf_point, const int32_t* d_n,
                                 int nframes, int cap, const int32_t* d_kf_order, int npoints, uint8_t* d_point_bad, int32_t* d_visible, int32_t* d_found,
                                 int32_t* d_replaced, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
                                 const uint8_t* d_obs_live, const int32_t* d_ref_obs, int obs_cap_out, int32_t* d_obs_start_out, int32_t* d_obs_frame_out,
                                 int32_t* d_obs_idx_out, int32_t* d_ref_obs_out, int32_t* d_edit_status, int32_t* d_touched, int select_bits, int sel_cap,
                                 int32_t* d_select_out, int32_t* d_info, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nedits < 0 || nframes < 0 || cap < 1 || npoints < 0 || nobs < 0 || obs_cap_out < 0 || sel_cap < 0 || !d_info || !d_obs_start_out ||
        (nedits && (!d_edits || !d_edit_status)) || (nframes && (!d_kf_point || !d_n)) ||
        (npoints && (!d_point_bad || !d_obs_start || !d_ref_obs || !d_ref_obs_out || !d_touched)) || (nobs && (!d_obs_frame || !d_obs_idx)) ||
        (obs_cap_out && (!d_obs_frame_out || !d_obs_idx_out)) || (sel_cap && !d_select_out))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_apply_map_edits_device");
    if (d_obs_start_out == d_obs_start || (nobs && (d_obs_frame_out == d_obs_frame || d_obs_idx_out == d_obs_idx)) || (npoints && d_ref_obs_out == d_ref_obs))
        return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits_device: an output aliases an input");
    if (nedits > PGORB_EDIT_MAX_LIST) return pg_ctx_fail(c, PGORB_E_LIMIT, "a list of more than PGORB_EDIT_MAX_LIST entries");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    if (nframes > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    if (npoints > (1 << 30) || (int64_t)nobs + nedits > 0x7FFFFFFF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 2^30 points or 2^31 observations");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const hipStream_t s = (hipStream_t)stream;
    const int ecap = nobs + std::min(nedits, PGORB_EDIT_MAX_EDITS);          // the lists that are left hold the input entries and the ADDs
    const size_t perPoint = edit_al((size_t)std::max(npoints, 1) * 4), perEdit = edit_al((size_t)(nedits + 1) * 4), perSort = edit_al((size_t)(std::min(nedits, PGORB_EDIT_MAX_EDITS) + 1) * 4), perPool = edit_al((size_t)std::max(ecap, 1) * 4);
    const size_t oCnt = 0, oPoint = edit_al(EC_COUNT * 4), oEdit = oPoint + 10 * perPoint, oPool = oEdit + perEdit + 2 * perSort, end = oPool + 5 * perPool;
    void* scr;
    int rc = pg_ctx_scratch(c, end, s, &scr);
    if (rc) return rc;
    uint8_t* b = (uint8_t*)scr;
    if (hipMemsetAsync(b + oCnt, 0, oPoint, s) != hipSuccess || hipMemsetAsync(b + oEdit, 0, oPool - oEdit, s) != hipSuccess)
        return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    auto pp = [&](int k) { return (int32_t*)(b + oPoint + k * perPoint); };
    auto pe = [&](int k) { return (int32_t*)(b + oEdit + (k ? perEdit + (k - 1) * perSort : 0)); };      // the status per list entry, then sorted and compFirst
    auto pl = [&](int k) { return (int32_t*)(b + oPool + k * perPool); };
    const PgEdit B = {d_edits, nedits, d_nedits, d_kf_point, d_n, nframes, cap, d_kf_order, npoints, d_point_bad, d_visible, d_found, d_replaced,
                      d_obs_start, d_obs_frame, d_obs_idx, nobs, d_obs_live, d_ref_obs, obs_cap_out, d_obs_start_out, d_obs_frame_out, d_obs_idx_out,
                      d_ref_obs_out, d_edit_status, d_touched, select_bits, sel_cap, d_select_out, d_info,
                      pp(0), pp(1), pp(2), pp(3), pp(4), pp(5), pp(6), pp(7), pp(8), pp(9), pe(1), pe(2), pe(0), ecap, pl(0), pl(1), pl(2), pl(3), pl(4),
                      (int32_t*)(b + oCnt)};
    const auto blocks = [](int n) { return dim3((unsigned)((std::max(n, 1) + EDIT_T - 1) / EDIT_T)); };
    if (npoints) hipLaunchKernelGGL(k_edit_init, blocks(npoints), dim3(EDIT_T), 0, s, B);
    if (nedits) {
        hipLaunchKernelGGL(k_edit_components, dim3(1), dim3(EDIT_CT), 0, s, B);
        hipLaunchKernelGGL(k_edit_bucket, dim3(1), dim3(EDIT_CT), 0, s, B);
        hipLaunchKernelGGL(k_edit_plan, dim3((unsigned)std::min(nedits, PGORB_EDIT_MAX_EDITS)), dim3(64), 0, s, B);
    }
    hipLaunchKernelGGL(k_edit_scan, dim3(1), dim3(EDIT_T), 0, s, B);
    if (ecap) hipLaunchKernelGGL(k_edit_mark, blocks(ecap), dim3(EDIT_T), 0, s, B);
    hipLaunchKernelGGL(k_edit_commit, blocks(std::max(std::max(npoints, ecap), nedits)), dim3(EDIT_T), 0, s, B);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_edit_* launch failed");
    return pg_ctx_scratch_done(c, s);
}

// ---- the host form: checked, then one synchronous call of the device form
int pgorb_apply_map_edits(pgorb_ctx* c, const pgorb_map_edit* edits, int nedits, int nkf, int32_t* const* kf_point, const int32_t* n, const int32_t* kf_order,
                          int npoints, uint8_t* point_bad, int32_t* visible, int32_t* found, int32_t* replaced, const int32_t* obs_start,
                          const int32_t* obs_frame, const int32_t* obs_idx, const uint8_t* obs_live, const int32_t* ref_obs, int obs_cap_out,
                          int32_t* obs_start_out, int32_t* obs_frame_out, int32_t* obs_idx_out, int32_t* ref_obs_out, int32_t* edit_status, int32_t* touched,
                          int select_bits, int sel_cap, int32_t* select_out, int32_t* info)
{
    if (!c) return PGORB_E_ARG;
    const char* bad = "bad argument to pgorb_apply_map_edits";
    if (nedits < 0 || nkf < 0 || npoints < 0 || obs_cap_out < 0 || sel_cap < 0 || !info || !obs_start_out || (nedits && (!edits || !edit_status)) ||
        (nkf && (!kf_point || !n)) || (npoints && (!point_bad || !obs_start || !ref_obs || !ref_obs_out || !touched)) ||
        (obs_cap_out && (!obs_frame_out || !obs_idx_out)) || (sel_cap && !select_out))
        return pg_ctx_fail(c, PGORB_E_ARG, bad);
    if (nedits > PGORB_EDIT_MAX_LIST) return pg_ctx_fail(c, PGORB_E_LIMIT, "a list of more than PGORB_EDIT_MAX_LIST entries");
    if (nkf > PGORB_COVIS_MAX_KF) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_COVIS_MAX_KF key frames");
    int cap = 1;
    for (int k = 0; k < nkf; k++) {
        if (n[k] < 0 || (n[k] && !kf_point[k])) return pg_ctx_fail(c, PGORB_E_ARG, bad);
        if (n[k] > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints");
        cap = std::max(cap, n[k]);
    }
    int real = 0;
    for (int e = 0; e < nedits; e++) {
        if (edits[e].op < PGORB_EDIT_NOP || edits[e].op > PGORB_EDIT_SET_REF) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: an unknown op");
        real += edits[e].op != PGORB_EDIT_NOP;
    }
    if (real > PGORB_EDIT_MAX_EDITS) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than PGORB_EDIT_MAX_EDITS edits that are not NOP");
    if (kf_order) {
        std::vector<uint8_t> seen((size_t)std::max(nkf, 1), 0);
        for (int k = 0; k < nkf; k++) {
            if (kf_order[k] < 0 || kf_order[k] >= nkf || seen[kf_order[k]]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: kf_order is not a permutation");
            seen[kf_order[k]] = 1;
        }
    }
    int nobs = 0;
    if (npoints) {
        if (obs_start[0] != 0) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: obs_start[0] must be 0");
        for (int p = 0; p < npoints; p++)
            if (obs_start[p + 1] < obs_start[p]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: obs_start decreases");
        nobs = obs_start[npoints];
        if (nobs && (!obs_frame || !obs_idx)) return pg_ctx_fail(c, PGORB_E_ARG, bad);
        std::vector<int32_t> seen((size_t)std::max(nkf, 1), -1);
        for (int p = 0; p < npoints; p++) {
            const int len = obs_start[p + 1] - obs_start[p];
            if (len && (ref_obs[p] < -1 || ref_obs[p] >= len)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: ref_obs is outside its list");
            for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
                if (obs_live && !obs_live[o]) continue;                            // a dead entry does not exist
                const int k = obs_frame[o];
                if (k < 0 || k >= nkf) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: an observation names a key frame out of range");
                if (obs_idx[o] < 0 || obs_idx[o] >= n[k]) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: an observation names a keypoint out of range");
                if (seen[k] == p) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: a list names a key frame twice");
                seen[k] = p;
            }
        }
    }
    {
        const auto overlap = [](const void* x, size_t xb, const void* y, size_t yb) {
            return x && y && xb && yb && (const uint8_t*)x < (const uint8_t*)y + yb && (const uint8_t*)y < (const uint8_t*)x + xb;
        };
        const struct { const void* p; size_t b; } outs[] = {{obs_start_out, (size_t)(npoints + 1) * 4}, {obs_frame_out, (size_t)obs_cap_out * 4},
                                                            {obs_idx_out, (size_t)obs_cap_out * 4}, {ref_obs_out, (size_t)npoints * 4}},
                                                  ins[] = {{obs_start, (size_t)(npoints + 1) * 4}, {obs_frame, (size_t)nobs * 4}, {obs_idx, (size_t)nobs * 4},
                                                           {ref_obs, (size_t)npoints * 4}, {obs_live, (size_t)nobs}};
        for (const auto& o : outs)
            for (const auto& i : ins)
                if (overlap(o.p, o.b, i.p, i.b)) return pg_ctx_fail(c, PGORB_E_ARG, "pgorb_apply_map_edits: an output aliases an input");
    }
    const int nf = std::max(nkf, 1), np = std::max(npoints, 1), no = std::max(nobs, 1), ne = std::max(nedits, 1), oc = std::max(obs_cap_out, 1), sc = std::max(sel_cap, 1);
    PgHostCall hc(c);
    const size_t oE = hc.region(PG_UP, (size_t)ne * sizeof(pgorb_map_edit)), oN = hc.region(PG_UP, (size_t)nf * 4), oOrd = hc.region(PG_UP, (size_t)nf * 4),
                 oOS = hc.region(PG_UP, (size_t)(npoints + 1) * 4), oOF = hc.region(PG_UP, (size_t)no * 4), oOI = hc.region(PG_UP, (size_t)no * 4),
                 oL = hc.region(PG_UP, no), oRef = hc.region(PG_UP, (size_t)np * 4),
                 oS = hc.region(PG_INOUT, (size_t)nf * cap * 4), oB = hc.region(PG_INOUT, np), oVi = hc.region(PG_INOUT, (size_t)np * 4),
                 oFo = hc.region(PG_INOUT, (size_t)np * 4), oRp = hc.region(PG_INOUT, (size_t)np * 4),
                 oSO = hc.region(PG_INOUT, (size_t)(npoints + 1) * 4), oFO = hc.region(PG_INOUT, (size_t)oc * 4), oIO = hc.region(PG_INOUT, (size_t)oc * 4),
                 oRO = hc.region(PG_INOUT, (size_t)np * 4), oSt = hc.region(PG_INOUT, (size_t)ne * 4), oT = hc.region(PG_INOUT, (size_t)np * 4),
                 oSel = hc.region(PG_INOUT, (size_t)sc * 4), oInfo = hc.region(PG_INOUT, PGORB_EDIT_INFO * 4);
    int rc;
    if ((rc = hc.begin())) return rc;
    int32_t* slots = hc.host<int32_t>(oS);
    for (int k = 0; k < nf; k++)
        for (int s = 0; s < cap; s++) slots[(size_t)k * cap + s] = (k < nkf && s < n[k]) ? kf_point[k][s] : -1;
    hc.put(oE, edits, (size_t)nedits * sizeof(pgorb_map_edit), 0, (size_t)ne * sizeof(pgorb_map_edit));
    hc.put(oN, n, (size_t)nkf * 4, 0, (size_t)nf * 4);
    hc.put(oOrd, kf_order, (size_t)nkf * 4, 0, (size_t)nf * 4);
    if (npoints) hc.put(oOS, obs_start, (size_t)(npoints + 1) * 4); else hc.put(oOS, nullptr, 0, 0, 4);
    hc.put(oOF, obs_frame, (size_t)nobs * 4, 0, (size_t)no * 4);
    hc.put(oOI, obs_idx, (size_t)nobs * 4, 0, (size_t)no * 4);
    if (obs_live) hc.put(oL, obs_live, nobs, 0, no); else memset(hc.host(oL), 1, no);
    hc.put(oRef, ref_obs, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oB, point_bad, npoints, 0, np);
    hc.put(oVi, visible, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oFo, found, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oRp, replaced, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oSO, obs_start_out, (size_t)(npoints + 1) * 4);
    hc.put(oFO, obs_frame_out, (size_t)obs_cap_out * 4, 0, (size_t)oc * 4);
    hc.put(oIO, obs_idx_out, (size_t)obs_cap_out * 4, 0, (size_t)oc * 4);
    hc.put(oRO, ref_obs_out, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oSt, edit_status, (size_t)nedits * 4, 0, (size_t)ne * 4);
    hc.put(oT, touched, (size_t)npoints * 4, 0, (size_t)np * 4);
    hc.put(oSel, select_out, (size_t)sel_cap * 4, 0, (size_t)sc * 4);
    hc.put(oInfo, info, PGORB_EDIT_INFO * 4);
    if ((rc = hc.run([&] {
            return pgorb_apply_map_edits_device(c, hc.dev<pgorb_map_edit>(oE), nedits, nullptr, hc.dev<int32_t>(oS), hc.dev<int32_t>(oN), nkf, cap,
                                                kf_order ? hc.dev<int32_t>(oOrd) : nullptr, npoints, hc.dev(oB), visible ? hc.dev<int32_t>(oVi) : nullptr,
                                                found ? hc.dev<int32_t>(oFo) : nullptr, replaced ? hc.dev<int32_t>(oRp) : nullptr, hc.dev<int32_t>(oOS),
                                                hc.dev<int32_t>(oOF), hc.dev<int32_t>(oOI), nobs, hc.dev(oL), hc.dev<int32_t>(oRef), obs_cap_out,
                                                hc.dev<int32_t>(oSO), hc.dev<int32_t>(oFO), hc.dev<int32_t>(oIO), hc.dev<int32_t>(oRO), hc.dev<int32_t>(oSt),
                                                hc.dev<int32_t>(oT), select_bits, sel_cap, hc.dev<int32_t>(oSel), hc.dev<int32_t>(oInfo), nullptr); }))) return rc;
    const int32_t* back = hc.host<int32_t>(oS);
    for (int k = 0; k < nkf; k++)
        if (n[k]) memcpy(kf_point[k], back + (size_t)k * cap, (size_t)n[k] * 4);
    if (npoints) {
        memcpy(point_bad, hc.host(oB), npoints);
        if (visible) memcpy(visible, hc.host(oVi), (size_t)npoints * 4);
        if (found) memcpy(found, hc.host(oFo), (size_t)npoints * 4);
        if (replaced) memcpy(replaced, hc.host(oRp), (size_t)npoints * 4);
        memcpy(ref_obs_out, hc.host(oRO), (size_t)npoints * 4);
        memcpy(touched, hc.host(oT), (size_t)npoints * 4);
    }
    memcpy(obs_start_out, hc.host(oSO), (size_t)(npoints + 1) * 4);
    if (obs_cap_out) { memcpy(obs_frame_out, hc.host(oFO), (size_t)obs_cap_out * 4); memcpy(obs_idx_out, hc.host(oIO), (size_t)obs_cap_out * 4); }
    if (nedits) memcpy(edit_status, hc.host(oSt), (size_t)nedits * 4);
    if (sel_cap) memcpy(select_out, hc.host(oSel), (size_t)sel_cap * 4);
    memcpy(info, hc.host(oInfo), PGORB_EDIT_INFO * 4);
    return info[0] == PGORB_EDIT_LIMIT ? 0 : info[2];
}

}  // extern "C"

// ---- the producers: each turns one step's output into edits at fixed positions, NOP where nothing happens, so that the list
// order is the reference's loop order
__device__ __forceinline__ void edit_put(pgorb_map_edit* out, int op, int a, int b, int c) { out->op = op; out->a = a; out->b = b; out->c = c; }

struct PgEditSrc {
    const int32_t* kfPoint; const int32_t* n; int nframes; int cap; int npoints; const uint8_t* pbad;
    const int32_t* obsStart; const int32_t* obsFrame; int nobs; const uint8_t* live;
};

// ProcessNewKeyFrame (LocalMapping.cc:142-161): a thread per slot of kf
__global__ __launch_bounds__(EDIT_T) void k_edit_from_keyframe(PgEditSrc T, int kf, pgorb_map_edit* edits, int32_t* slotClass)
{
    const int i = blockIdx.x * EDIT_T + threadIdx.x;
    if (i >= T.cap) return;
    int cls = 0, P = -1;
    const bool kfOk = kf >= 0 && kf < T.nframes;
    const int n = kfOk ? min(max(T.n[kf], 0), T.cap) : 0;
    if (i < n) {
        const int32_t* row = T.kfPoint + (int64_t)kf * T.cap;
        P = row[i];
        if (P >= 0 && P < T.npoints && !T.pbad[P]) {
            bool in = false;                                                       // IsInKeyFrame: by the point's list, or made so by a lower slot's ADD
            const int a = T.obsStart[P], b = T.obsStart[P + 1];
            if (a >= 0 && b >= a && b <= T.nobs)
                for (int o = a; o < b && !in; o++) in = (!T.live || T.live[o]) && T.obsFrame[o] == kf;
            for (int j = 0; j < i && !in; j++) in = row[j] == P;
            cls = in ? 2 : 1;
        }
    }
    if (cls == 1) edit_put(edits + i, PGORB_EDIT_ADD, P, kf, i); else edit_put(edits + i, PGORB_EDIT_NOP, 0, 0, 0);
    slotClass[i] = cls;
}

// Optimizer.cc:748-757: a thread per CSR position
__global__ __launch_bounds__(EDIT_T) void k_edit_from_lba_erase(int npoints, const int32_t* __restrict__ obsStart, const int32_t* __restrict__ obsFrame, int nobs,
                                                                const uint8_t* __restrict__ erase, pgorb_map_edit* edits)
{
    const int j = blockIdx.x * EDIT_T + threadIdx.x;
    if (j >= nobs) return;
    int p = -1;
    if (erase[j]) {
        int lo = 0, hi = npoints;                                                  // the last p with obs_start[p] <= j
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (obsStart[mid + 1] <= j) lo = mid + 1; else hi = mid; }
        if (lo < npoints && obsStart[lo] <= j) p = lo;
    }
    if (p >= 0) edit_put(edits + j, PGORB_EDIT_ERASE, p, obsFrame[j], 0); else edit_put(edits + j, PGORB_EDIT_NOP, 0, 0, 0);
}

// LoopClosing.cc:520-537: a thread per slot of cur_kf, from the entry state (an occupant lists cur_kf only at its own slot)
__global__ __launch_bounds__(EDIT_T) void k_edit_from_loop_matches(const int32_t* __restrict__ kfPoint, const int32_t* __restrict__ n, int nframes, int cap,
                                                                   int npoints, int curKf, const int32_t* __restrict__ matched, pgorb_map_edit* edits)
{
    const int i = blockIdx.x * EDIT_T + threadIdx.x;
    if (i >= cap) return;
    const int nk = (curKf >= 0 && curKf < nframes) ? min(max(n[curKf], 0), cap) : 0;
    const int m = i < nk ? matched[i] : -1;
    if (m < 0 || m >= npoints) { edit_put(edits + i, PGORB_EDIT_NOP, 0, 0, 0); return; }
    const int occ = kfPoint[(int64_t)curKf * cap + i];
    if (occ >= 0 && occ < npoints) edit_put(edits + i, PGORB_EDIT_REPLACE, occ, m, 0); else edit_put(edits + i, PGORB_EDIT_ADD, m, curKf, i);
}

// ORBmatcher.cc:961-979 (replacePoint == NULL) and LoopClosing.cc:601-615: a thread per query
__global__ __launch_bounds__(EDIT_T) void k_edit_from_fuse(const int32_t* __restrict__ kfPoint, const int32_t* __restrict__ n, int nframes, int cap, int npoints,
                                                           int kf, int qcap, const int32_t* __restrict__ nqPtr, const int32_t* __restrict__ queries,
                                                           const int32_t* __restrict__ action, const int32_t* __restrict__ bestIdx,
                                                           const int32_t* __restrict__ replacePoint, pgorb_map_edit* edits)
{
    const int q = blockIdx.x * EDIT_T + threadIdx.x;
    if (q >= qcap) return;
    pgorb_map_edit nop = {PGORB_EDIT_NOP, 0, 0, 0};
    edits[q] = nop;
    if (replacePoint) edits[qcap + q] = nop;
    const int nq = min(max(nqPtr[0], 0), qcap);
    const int nk = (kf >= 0 && kf < nframes) ? min(max(n[kf], 0), cap) : 0;
    if (q >= nq) return;
    const int P = queries[q], act = action[q], s = bestIdx[q];
    if (P < 0 || P >= npoints || s < 0 || s >= nk) return;
    if (act == PGORB_FUSE_ADDED) { edit_put(edits + q, PGORB_EDIT_ADD, P, kf, s); return; }
    if (replacePoint) {                                                            // Fuse runs to its end before the replacements
        if (act == PGORB_FUSE_REPLACE_REQUESTED) edit_put(edits + qcap + q, PGORB_EDIT_REPLACE, replacePoint[q], P, 0);
        return;
    }
    if (act != PGORB_FUSE_MERGED_INTO_KF_POINT && act != PGORB_FUSE_REPLACED_KF_POINT) return;
    int occ = kfPoint[(int64_t)kf * cap + s];                                      // the slot's running occupant
    for (int j = q - 1; j >= 0; j--)
        if (bestIdx[j] == s && queries[j] >= 0 && queries[j] < npoints && (action[j] == PGORB_FUSE_ADDED || action[j] == PGORB_FUSE_REPLACED_KF_POINT)) {
            occ = queries[j];
            break;
        }
    if (act == PGORB_FUSE_MERGED_INTO_KF_POINT) edit_put(edits + q, PGORB_EDIT_REPLACE, P, occ, 0);
    else edit_put(edits + q, PGORB_EDIT_REPLACE, occ, P, 0);
}

// the ids of every list, ascending: a thread per point, an insertion sort into the output
__global__ __launch_bounds__(EDIT_T) void k_edit_observation_ids(int npoints, const int32_t* __restrict__ obsStart, const int32_t* __restrict__ obsFrame, int nobs,
                                                                 const uint64_t* __restrict__ kfId, int nframes, uint64_t* __restrict__ out)
{
    const int p = blockIdx.x * EDIT_T + threadIdx.x;
    if (p >= npoints) return;
    const int a = obsStart[p], b = obsStart[p + 1];
    if (a < 0 || b < a || b > nobs) return;
    for (int o = a; o < b; o++) {
        const int f = obsFrame[o];
        const uint64_t id = (f >= 0 && f < nframes) ? kfId[f] : ~0ull;
        int w = o;
        while (w > a && out[w - 1] > id) { out[w] = out[w - 1]; w--; }
        out[w] = id;
    }
}

extern "C" {

#define EDIT_BEGIN(fn)                                                                                             \
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");   \
    const hipStream_t s = (hipStream_t)stream;                                                                     \
    const char* const fnName = fn;                                                                                 \
    const auto blocks = [](int n) { return dim3((unsigned)((std::max(n, 1) + EDIT_T - 1) / EDIT_T)); }
#define EDIT_END()                                                                                                 \
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, (std::string(fnName) + ": launch failed").c_str());   \
    return 0

int pgorb_map_edits_from_keyframe_device(pgorb_ctx* c, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap, int npoints,
                                         const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs,
                                         const uint8_t* d_obs_live, int kf, pgorb_map_edit* d_edits, int32_t* d_slot_class, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 1 || cap < 1 || npoints < 0 || nobs < 0 || kf < 0 || kf >= nframes || !d_kf_point || !d_n || !d_edits || !d_slot_class ||
        (npoints && (!d_point_bad || !d_obs_start)) || (nobs && !d_obs_frame))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_edits_from_keyframe_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    EDIT_BEGIN("pgorb_map_edits_from_keyframe_device");
    const PgEditSrc T = {d_kf_point, d_n, nframes, cap, npoints, d_point_bad, d_obs_start, d_obs_frame, nobs, d_obs_live};
    hipLaunchKernelGGL(k_edit_from_keyframe, blocks(cap), dim3(EDIT_T), 0, s, T, kf, d_edits, d_slot_class);
    EDIT_END();
}

int pgorb_map_edits_from_lba_erase_device(pgorb_ctx* c, int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint8_t* d_erase,
                                          pgorb_map_edit* d_edits, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (npoints < 0 || nobs < 0 || (npoints && !d_obs_start) || (nobs && (!d_obs_frame || !d_erase || !d_edits)))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_edits_from_lba_erase_device");
    EDIT_BEGIN("pgorb_map_edits_from_lba_erase_device");
    if (nobs) hipLaunchKernelGGL(k_edit_from_lba_erase, blocks(nobs), dim3(EDIT_T), 0, s, npoints, d_obs_start, d_obs_frame, nobs, d_erase, d_edits);
    EDIT_END();
}

int pgorb_map_edits_from_loop_matches_device(pgorb_ctx* c, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap, int npoints, int cur_kf,
                                             const int32_t* d_matched, pgorb_map_edit* d_edits, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 1 || cap < 1 || npoints < 0 || cur_kf < 0 || cur_kf >= nframes || !d_kf_point || !d_n || !d_matched || !d_edits)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_edits_from_loop_matches_device");
    if (cap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame");
    EDIT_BEGIN("pgorb_map_edits_from_loop_matches_device");
    hipLaunchKernelGGL(k_edit_from_loop_matches, blocks(cap), dim3(EDIT_T), 0, s, d_kf_point, d_n, nframes, cap, npoints, cur_kf, d_matched, d_edits);
    EDIT_END();
}

int pgorb_map_edits_from_fuse_device(pgorb_ctx* c, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap, int npoints, int kf, int qcap,
                                     const int32_t* d_nq, const int32_t* d_queries, const int32_t* d_action, const int32_t* d_best_idx,
                                     const int32_t* d_replace_point, pgorb_map_edit* d_edits, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (nframes < 1 || cap < 1 || npoints < 0 || kf < 0 || kf >= nframes || qcap < 1 || !d_kf_point || !d_n || !d_nq || !d_queries || !d_action ||
        !d_best_idx || !d_edits)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_map_edits_from_fuse_device");
    if (cap > 16000 || qcap > 16000) return pg_ctx_fail(c, PGORB_E_LIMIT, "more than 16000 keypoints per frame or queries");
    EDIT_BEGIN("pgorb_map_edits_from_fuse_device");
    hipLaunchKernelGGL(k_edit_from_fuse, blocks(qcap), dim3(EDIT_T), 0, s, d_kf_point, d_n, nframes, cap, npoints, kf, qcap, d_nq, d_queries, d_action,
                       d_best_idx, d_replace_point, d_edits);
    EDIT_END();
}

int pgorb_observation_ids_device(pgorb_ctx* c, int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint64_t* d_kf_id,
                                 int nframes, uint64_t* d_obs_kf_out, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (npoints < 0 || nobs < 0 || nframes < 0 || (npoints && !d_obs_start) || (nobs && (!d_obs_frame || !d_obs_kf_out)) || (nframes && !d_kf_id))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_observation_ids_device");
    EDIT_BEGIN("pgorb_observation_ids_device");
    if (npoints && nobs) hipLaunchKernelGGL(k_edit_observation_ids, blocks(npoints), dim3(EDIT_T), 0, s, npoints, d_obs_start, d_obs_frame, nobs, d_kf_id, nframes, d_obs_kf_out);
    EDIT_END();
}

}  // extern "C"
