// cand_lists.h -- the candidate lists between the two passes of the grid-window matchers: SearchForInitialization (init_match.hip)
// and the SearchByProjection forms (window_match.hip; track.hip reaches them through proj_match.h).  The list format, the walk of a
// query's grid window that fills a list, the reading of a stored list and the host's side of a call's lists are here and nowhere else.
#pragma once
#include "match_common.h"
#include <assert.h>

// keypoints of a frame / queries of a pair a two-pass matcher takes (every entry point checks it before anything else is sized):
// the index fields of the stored entries and the 16-bit candidate lists in LDS are laid out for it
#define LIST_MAX_N 16000

// ---- candidate lists of the two-pass matchers (round 4: variable length) -----------------------------------------------
// Pass A stores EVERY surviving candidate of a query in the reference's scan order: the first LIST_K in the query's fixed slots,
// the rest in the pair's pool (one atomic per query that needs it).  Rounds 2-3 capped the lists at 64 and re-evaluated denser
// queries in place inside the sequential pass -- the initialisation workload's cliff.  Only when a pair's pool is full (an
// average of LIST_K + LIST_POOL candidates per query) is a query still evaluated in place (count LIST_OVER).
#define LIST_K 64
#define LIST_POOL 256
#define LIST_OVER 0xFFFFu
struct PgLists {
    uint32_t* fixed;             // [rows][LIST_K]
    uint16_t* cnt;               // [rows]   survivors of the query (LIST_OVER: evaluate in place)
    uint32_t* ovf;               // [rows]   where the query's entries LIST_K.. start in its pair's pool
    uint32_t* pool;              // [npairs][poolPerPair]
    int32_t*  poolTop;           // [npairs] (zeroed before pass A)
    uint32_t  poolPerPair;
};

static PgGridWin pg_grid_win(float min_x, float max_x, float min_y, float max_y)
{
    return PgGridWin{min_x, min_y, (float)GRID_COLS / (max_x - min_x), (float)GRID_ROWS / (max_y - min_y)};
}

// scratch layout for npairs x rowsPerPair rows; returns the bytes needed
static size_t pg_lists_layout(void* scratch, int npairs, int rowsPerPair, PgLists* L)
{
    const size_t rows = (size_t)npairs * rowsPerPair;
    uint8_t* b = (uint8_t*)scratch;
    PgCarve cv;
    L->poolPerPair = (uint32_t)((size_t)rowsPerPair * LIST_POOL);
    L->poolTop = (int32_t*)(b + cv.take((size_t)npairs * 4));
    L->fixed = (uint32_t*)(b + cv.take(rows * LIST_K * 4));
    L->cnt = (uint16_t*)(b + cv.take(rows * 2));
    L->ovf = (uint32_t*)(b + cv.take(rows * 4));
    L->pool = (uint32_t*)(b + cv.take((size_t)npairs * L->poolPerPair * 4));
    return cv.o;
}

// What a call does on the host before its two passes KA and KB: the device, their dynamic LDS (`ldsMsg`: the family's refusal), and ONE
// block of the matchers' scratch arena holding the candidate lists of npairs x rowsPerPair queries, the pools empty, and behind them
// `extraBytes` for the caller's own arrays (*extra, 256-byte aligned).  The caller ends with pg_ctx_scratch_done.
template <auto KA, auto KB>
static int pg_lists_acquire(pgorb_ctx* c, int npairs, int rowsPerPair, size_t ldsA, size_t ldsB, const char* ldsMsg, size_t extraBytes,
                            hipStream_t stream, PgLists* L, void** extra)
{
    assert(rowsPerPair <= LIST_MAX_N);                       // (the entry points refuse more, each with its own message)
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    if (!pg_raise_lds<KA>(c, ldsA) || !pg_raise_lds<KB>(c, ldsB)) return pg_ctx_fail(c, PGORB_E_LIMIT, ldsMsg);
    const size_t lists = pg_lists_layout(nullptr, npairs, rowsPerPair, L) + 256;
    void* scratch;
    const int rc = pg_ctx_scratch(c, lists + extraBytes, stream, &scratch);
    if (rc) return rc;
    pg_lists_layout(scratch, npairs, rowsPerPair, L);
    if (extra) *extra = (uint8_t*)scratch + lists;
    if (hipMemsetAsync(L->poolTop, 0, (size_t)npairs * 4, stream) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipMemsetAsync failed");
    return 0;
}

// ---- pass A: from a query's grid window to its stored list ------------------------------------------------------------------------
// GetFeaturesInArea's vIndices before its filters, by one wave: the cells cx0..cx1 x cy0..cy1 of a frame's grid (CSR: start, idx) in
// (column, row) order, each cell's entries in insertion order, into this wave's candList in LDS.  Returns their number M; the list is
// visible to every lane on return.
__device__ __forceinline__ int pg_window_gather(const int32_t* __restrict__ start, const int32_t* __restrict__ idx, int cx0, int cx1, int cy0,
                                                int cy1, uint16_t* candList, int lane)
{
    const int ncy = cy1 - cy0 + 1, T = (cx1 - cx0 + 1) * ncy;
    int M = 0;
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        int s0 = 0, cnt = 0;
        if (t < T) {
            const int c = (cx0 + t / ncy) * GRID_ROWS + cy0 + t % ncy;
            s0 = start[c]; cnt = start[c + 1] - s0;
        }
        const int incl = wave_incl_scan(cnt, lane);
        const int off = M + incl - cnt;
#pragma clang loop interleave(disable)       // (a second copy of this loop in flight costs pass A 14 VGPRs: all it has left at 8 waves a SIMD)
        for (int j = 0; j < cnt; j++) candList[off + j] = (uint16_t)idx[s0 + j];
        M += __builtin_amdgcn_readlane(incl, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return M;
}

// the tail of a query's wave: `total` survivors are about to be written.  Reserves pool space when they do not fit the
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

// The list of query `row` of pair p from its M gathered candidates: entry(k, e) says whether candidate k survives the reference's
// filters and, if so, sets its 32-bit entry e (for a lane that does not survive it must not cost the distance's loads: select, do not
// return early).  Survivors are stored in order.  Those beyond the fixed slots go to the pair's pool, reserved in one piece the moment
// the 65th survivor turns up -- for what is left of the window's M keypoints, an upper bound (counting the survivors first cost a
// second pass over the keypoints, and reserving for every query with M > 64 an atomic per query on the pair's counter: + 25 % /
// + 100 % on the whole matcher).
template <class Entry>
__device__ __forceinline__ void pg_list_build(const PgLists& Ls, int64_t row, int p, int M, int lane, Entry&& entry)
{
    int total = 0;
    bool over = false, reserved = false;
    uint32_t ovf = 0;
    uint32_t* out = Ls.fixed + row * LIST_K;
    uint32_t* outPool = Ls.pool + (size_t)p * Ls.poolPerPair;
    for (int base = 0; base < M; base += 64) {
        const int k = base + lane;
        uint32_t e = 0u;
        const bool ok = k < M && entry(k, e);
        const unsigned long long m = __ballot(ok);
        const int pos = total + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        total += __popcll(m);
        if (total > LIST_K && !reserved) { ovf = pg_list_reserve(Ls, p, LIST_K + (M - base), lane, over); reserved = true; }     // (wave-uniform)
        if (ok) { if (pos < LIST_K) out[pos] = e; else if (!over) outPool[ovf + (uint32_t)(pos - LIST_K)] = e; }
    }
    if (lane == 0) { Ls.cnt[row] = (uint16_t)(over ? LIST_OVER : total); Ls.ovf[row] = ovf; }
}

// ---- pass B: reading a stored list, or -- the pair's pool was full -- the window again ---------------------------------------------
// where the entries LIST_K.. of a query of pair p start, given the query's Ls.ovf
__device__ __forceinline__ const uint32_t* pg_list_tail(const PgLists& Ls, int p, uint32_t ovf) { return Ls.pool + (size_t)p * Ls.poolPerPair + ovf; }
// A stored list of `count` entries 64 at a time, one entry per lane: chunk 0 is `e0`, the query's fixed slots as the caller prefetched
// them, the further chunks come from `tail` (pg_list_tail; not read when count <= LIST_K).  body(chunk, entry, inRange) -- inRange:
// chunk * 64 + lane < count, the entry of any other lane is not one -- returns false to end the walk.
template <class Body>
__device__ __forceinline__ void pg_list_chunks(int count, uint32_t e0, const uint32_t* tail, int lane, Body&& body)
{
    for (int ch = 0; ch * 64 < count; ch++) {
        const uint32_t ee = ch == 0 ? e0 : tail[(uint32_t)(ch - 1) * 64u + (uint32_t)lane];
        if (!body(ch, ee, ch * 64 + lane < count)) break;
    }
}

// The evaluation in place of a query marked LIST_OVER: the wave visits the window's keypoints cell by cell in the reference's
// (column, row, insertion) order, 64 entries of a cell at a time: visit(i2, pos), pos = the keypoint's position in the scan (what
// pg_window_gather would have made its index in candList).
template <class Visit>
__device__ __forceinline__ void pg_window_walk(const int32_t* start, const int32_t* idx, int cx0, int cx1, int cy0, int cy1, int lane, Visit&& visit)
{
    int posBase = 0;
    for (int ix = cx0; ix <= cx1; ix++)
        for (int iy = cy0; iy <= cy1; iy++) {
            const int c = ix * GRID_ROWS + iy, s0 = start[c], cnt = start[c + 1] - s0;
            for (int k = lane; k < cnt; k += 64) visit(idx[s0 + k], posBase + k);
            posBase += cnt;
        }
}
