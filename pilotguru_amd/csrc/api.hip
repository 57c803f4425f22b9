// api.hip -- the context of libpgorb.so: pgorb_create / pgorb_destroy with the constructor tables of ORB_SLAM2::ORBextractor
// (thirdparty/orb-slam2/src/ORBextractor.cc:410-470), the options, the pg_ctx_* services of the kernel files, the page-locked
// helpers, the Hamming entries.  The per-frame-size plan is in plan.hip, the launch order and pgorb_extract* in extract.hip,
// pgorb_stream_* in stream.hip; the four share pgorb_ctx.h.  Everything per-pixel / per-keypoint runs in the HIP kernels; there
// is no CPU fallback.
#include "pgorb_ctx.h"

#include <stdarg.h>

static thread_local std::string g_create_error;

int fail(pgorb_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

int ensure(pgorb_ctx* c, Arena& a, size_t bytes)
{
    if (a.bytes >= bytes && a.p) return 0;
    if (a.p) { (void)hipFree(a.p); a.p = nullptr; a.bytes = 0; }
    bytes = (bytes + 4095) & ~(size_t)4095;
    PG_HIP(c, hipMalloc(&a.p, bytes));
    a.bytes = bytes;
    return 0;
}

namespace {

// Every option of pgorb_set_option / pgorb_get_option: where the context keeps it, which values it takes (no rule: all) with the
// message for the others, and what it keeps of a value (no rule: the value).  copy_tunables hands all of them to a stream's lanes.
struct PgOption {
    const char* key;
    int& (*at)(pgorb_ctx* c);
    bool (*valid)(int v);
    const char* error;
    int (*store)(int v);
};
#define PG_OPT_AT(field) [](pgorb_ctx* c) -> int& { return c->field; }
const PgOption kOptions[] = {
    {"matcher", PG_OPT_AT(mx.popcount), nullptr, nullptr,
     [](int v) { return v ? 1 : pg_match_default_opts().popcount; }},                                  // 0 = what the environment says
    {"match_mode", PG_OPT_AT(mx.mode), [](int v) { return v >= -1 && v <= 2; }, "match_mode must be -1, 0, 1 or 2", nullptr},
    {"fast_tile_pitch", PG_OPT_AT(fastTilePitch), [](int v) { return v == 0 || (v >= 48 && v <= 128 && v % 16 == 0); },
     "fast_tile_pitch must be 0 (automatic) or 48, 64, ... 128", nullptr},
    {"fast_waves_per_block", PG_OPT_AT(fastWpb), [](int v) { return v == 1 || v == 2 || v == 4; },
     "fast_waves_per_block must be 1, 2 or 4", nullptr},
    {"fast_cells_per_wave", PG_OPT_AT(fastCpw), [](int v) { return v >= 1 && v <= 64; }, "fast_cells_per_wave must be 1 ... 64", nullptr},
    {"quadtree_threads", PG_OPT_AT(qtThreads), [](int v) { return v == 0 || v == 256 || v == 512 || v == 1024; },
     "quadtree_threads must be 0 (automatic), 256, 512 or 1024", nullptr},
    {"quadtree_split", PG_OPT_AT(qtSplit), [](int v) { return v >= 0 && v <= 2; },
     "quadtree_split must be 0 (one launch), 1 (two) or 2 (automatic)", nullptr},
    {"fused_levels", PG_OPT_AT(fused), nullptr, nullptr, [](int v) { return v ? 1 : 0; }},
    {"pipeline_pyramid", PG_OPT_AT(pipePyr), nullptr, nullptr, [](int v) { return v ? 1 : 0; }},
    {"pipeline_levels", PG_OPT_AT(pipeLev), nullptr, nullptr, [](int v) { return v & ((1 << PG_MAXL) - 2); }},
    {"pipeline_levels_priority", PG_OPT_AT(pipeLevPrio), nullptr, nullptr, [](int v) { return v ? 1 : 0; }},
};
#undef PG_OPT_AT

const PgOption* find_option(const char* key)
{
    for (const PgOption& o : kOptions)
        if (!strcmp(key, o.key)) return &o;
    return nullptr;
}

}  // namespace

void copy_tunables(pgorb_ctx* dst, pgorb_ctx* src)
{
    for (const PgOption& o : kOptions) o.at(dst) = o.at(src);
}

// ---- the context services of pgorb_internal.h -----------------------------------------------
int pg_ctx_fail(pgorb_ctx* c, int code, const char* msg) { return fail(c, code, "%s", msg); }
int pg_ctx_device(pgorb_ctx* c) { return c->prm.device; }
int pg_ctx_stage(pgorb_ctx* c, PgStage which, size_t bytes, void** p)
{
    Arena* a = which == PG_STAGE_A ? &c->stageA : which == PG_STAGE_SFI ? &c->stageSfi : &c->stageOut;
    PG_HIP(c, hipSetDevice(c->prm.device));
    int rc = ensure(c, *a, bytes);
    if (rc) return rc;
    *p = a->p;
    return 0;
}
// The matchers' scratch arena (lists, bins) for work queued on stream `s`: SearchForInitialization, the projection searches and
// SearchByBoW share ONE arena per context, and a caller may queue them on different streams -- the new user waits for the
// previous user's event (round-3 advisory: BoW's memset of the bins could overtake a projection call still reading its lists).
// pg_ctx_scratch_done records the event after the last launch that touches the arena.
int pg_ctx_scratch(pgorb_ctx* c, size_t bytes, hipStream_t s, void** p)
{
    int rc = pg_ctx_stage(c, PG_STAGE_SFI, bytes, p);
    if (rc) return rc;
    if (c->sfiUsed && c->sfiStream != s) PG_HIP(c, hipStreamWaitEvent(s, c->evSfi, 0));
    return 0;
}
int pg_ctx_scratch_done(pgorb_ctx* c, hipStream_t s)
{
    if (!c->evSfi) PG_HIP(c, hipEventCreateWithFlags(&c->evSfi, hipEventDisableTiming));
    PG_HIP(c, hipEventRecord(c->evSfi, s));
    c->sfiStream = s; c->sfiUsed = true;
    return 0;
}
int pg_ctx_pinned(pgorb_ctx* c, size_t bytes, void** p)
{
    if (c->pinnedBytes < bytes) {
        PG_HIP(c, hipSetDevice(c->prm.device));
        if (c->pinned) (void)hipHostFree(c->pinned);
        c->pinned = nullptr; c->pinnedBytes = 0;
        const size_t want = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
        PG_HIP(c, hipHostMalloc(&c->pinned, want, hipHostMallocDefault));
        c->pinnedBytes = want;
    }
    *p = c->pinned;
    return 0;
}
// Sim3Solver::SetRansacParameters (Sim3Solver.cc:114-138) for N correspondences, in the reference's own expression: the host's log,
// and pow of the float epsilon promoted to double.  N == 0 divides by zero there; iterate() returns before the value is used.
int pg_sim3_cap(float probability, int min_inliers, int max_iterations, int N)
{
    const double mRansacProb = probability;
    int nIterations;
    if (min_inliers == N) nIterations = 1;
    else if (N <= 0) nIterations = 1;
    else {
        const float epsilon = (float)min_inliers / N;
        const double v = ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
        nIterations = (v != v || v >= 2147483648.0 || v < -2147483648.0) ? (-2147483647 - 1) : (int)v;      // cvttsd2si
    }
    return std::max(1, std::min(nIterations, max_iterations));
}
// The table of those caps for N = 0 .. max_n, kept on the device and re-made when the parameters change or max_n grows.  Re-making
// it waits for the device first: a call still queued on another stream may be reading the old table.
int pg_ctx_sim3_caps(pgorb_ctx* c, float probability, int min_inliers, int max_iterations, int max_n, const int32_t** d_caps)
{
    const int entries = max_n + 1;
    if (!(c->sim3Caps.p && c->sim3Prob == probability && c->sim3MinInliers == min_inliers && c->sim3MaxIts == max_iterations &&
          c->sim3Entries >= entries)) {
        PG_HIP(c, hipSetDevice(c->prm.device));
        std::vector<int32_t> t((size_t)entries);
        for (int N = 0; N < entries; N++) t[N] = pg_sim3_cap(probability, min_inliers, max_iterations, N);
        PG_HIP(c, hipDeviceSynchronize());
        c->sim3Entries = 0;
        int rc = ensure(c, c->sim3Caps, (size_t)entries * 4);
        if (rc) return rc;
        PG_HIP(c, hipMemcpy(c->sim3Caps.p, t.data(), (size_t)entries * 4, hipMemcpyHostToDevice));
        c->sim3Prob = probability; c->sim3MinInliers = min_inliers; c->sim3MaxIts = max_iterations; c->sim3Entries = entries;
    }
    *d_caps = (const int32_t*)c->sim3Caps.p;
    return 0;
}
// PnPsolver::SetRansacParameters (src/PnPsolver.cc:121-157) for N correspondences: the adjusted mRansacMinInliers and mRansacMaxIts.
// int(N*epsilon) is a float product truncated; epsilon is raised to (float)min/N; pow takes the float epsilon as a double; a value
// no int holds converts as cvttsd2si does
void pg_pnp_ransac(float probability, int min_inliers, int max_iterations, int min_set, float epsilon, int N, int32_t* min_out, int32_t* cap_out)
{
    const double mRansacProb = probability;
    float mRansacEpsilon = epsilon;
    int nMinInliers = (int)(N * mRansacEpsilon);
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (mRansacEpsilon < (float)nMinInliers / N) mRansacEpsilon = (float)nMinInliers / N;
    int nIterations;
    if (nMinInliers == N) nIterations = 1;
    else {
        const double v = ceil(log(1 - mRansacProb) / log(1 - pow((double)mRansacEpsilon, 3.0)));
        nIterations = (v != v || v >= 2147483648.0 || v < -2147483648.0) ? (-2147483647 - 1) : (int)v;
    }
    *min_out = nMinInliers;
    *cap_out = std::max(1, std::min(nIterations, max_iterations));
}
// The table of those pairs for N = 0 .. max_n on the device, kept and re-made as pg_ctx_sim3_caps keeps its own
int pg_ctx_pnp_table(pgorb_ctx* c, float probability, int min_inliers, int max_iterations, int min_set, float epsilon, int max_n, const int32_t** d_table)
{
    const int entries = max_n + 1;
    if (!(c->pnpTable.p && c->pnpProb == probability && c->pnpMinInliers == min_inliers && c->pnpMaxIts == max_iterations &&
          c->pnpMinSet == min_set && c->pnpEpsilon == epsilon && c->pnpEntries >= entries)) {
        PG_HIP(c, hipSetDevice(c->prm.device));
        std::vector<int32_t> t((size_t)entries * 2);
        for (int N = 0; N < entries; N++) pg_pnp_ransac(probability, min_inliers, max_iterations, min_set, epsilon, N, &t[2 * N], &t[2 * N + 1]);
        PG_HIP(c, hipDeviceSynchronize());
        c->pnpEntries = 0;
        int rc = ensure(c, c->pnpTable, (size_t)entries * 8);
        if (rc) return rc;
        PG_HIP(c, hipMemcpy(c->pnpTable.p, t.data(), (size_t)entries * 8, hipMemcpyHostToDevice));
        c->pnpProb = probability; c->pnpMinInliers = min_inliers; c->pnpMaxIts = max_iterations; c->pnpMinSet = min_set; c->pnpEpsilon = epsilon;
        c->pnpEntries = entries;
    }
    *d_table = (const int32_t*)c->pnpTable.p;
    return 0;
}
// the header of a vocabulary blob of `nbytes` bytes at `src` (bow.hip, blob layout) into `hdr`, checked: magic, version, and that the sections the
// header implies fit; the structure itself is checked by pgorb_vocab_from_blob / the loader on the host path and by
// k_vocab_validate on the device path
static int vocab_header_ok(pgorb_ctx* c, const void* src, size_t nbytes, bool src_on_device, hipStream_t s, int32_t* hdr)
{
    if (src_on_device) {
        PG_HIP(c, hipMemcpyAsync(hdr, src, 64, hipMemcpyDeviceToHost, s));
        PG_HIP(c, hipStreamSynchronize(s));
    } else memcpy(hdr, src, 64);
    if (hdr[0] != 0x43564750 || hdr[1] != 1 || hdr[4] < 2)
        return fail(c, PGORB_E_ARG, "not a pgorb vocabulary blob");
    const size_t n = (size_t)hdr[4];
    auto pad = [](size_t v) { return (v + 63) / 64 * 64; };
    size_t need = 64;
    need = pad(need + n * 32); need = pad(need + n * 8);
    for (int k = 0; k < 4; k++) need = pad(need + n * 4);
    need = pad(need + (n - 1) * 4);
    if (nbytes < need)
        return fail(c, PGORB_E_ARG, "vocabulary blob truncated: %zu bytes, header implies %zu", nbytes, need);
    return 0;
}
int pg_ctx_vocab_store(pgorb_ctx* c, const void* src, size_t nbytes, bool src_on_device, hipStream_t s)
{
    PG_HIP(c, hipSetDevice(c->prm.device));
    int32_t hdr[16];
    int rc = vocab_header_ok(c, src, nbytes, src_on_device, s, hdr);
    if (rc) return rc;
    if ((rc = ensure(c, c->vocab, nbytes))) return rc;
    if (src_on_device) PG_HIP(c, hipMemcpyAsync(c->vocab.p, src, nbytes, hipMemcpyDeviceToDevice, s));
    else PG_HIP(c, hipMemcpy(c->vocab.p, src, nbytes, hipMemcpyHostToDevice));
    c->vocabK = hdr[2]; c->vocabL = hdr[3]; c->vocabNodes = hdr[4]; c->vocabScoring = hdr[6]; c->vocabWeighting = hdr[7];
    return 0;
}
// The receive side of the vocabulary broadcast (comm.hip): room for `nbytes` in the context's vocabulary arena (the collective
// writes there directly, no second copy), then -- once the bytes have landed on stream `s` -- the header checks and the fields.
int pg_ctx_vocab_reserve(pgorb_ctx* c, size_t nbytes, void** p)
{
    PG_HIP(c, hipSetDevice(c->prm.device));
    pg_ctx_vocab_drop(c);
    int rc = ensure(c, c->vocab, nbytes);
    if (rc) return rc;
    *p = c->vocab.p;
    return 0;
}
int pg_ctx_vocab_commit(pgorb_ctx* c, size_t nbytes, hipStream_t s)
{
    PG_HIP(c, hipSetDevice(c->prm.device));
    int32_t hdr[16];
    if (int rc = vocab_header_ok(c, c->vocab.p, nbytes, true, s, hdr)) return rc;
    c->vocabK = hdr[2]; c->vocabL = hdr[3]; c->vocabNodes = hdr[4]; c->vocabScoring = hdr[6]; c->vocabWeighting = hdr[7];
    return 0;
}
void pg_ctx_vocab_drop(pgorb_ctx* c) { c->vocabK = c->vocabL = c->vocabNodes = 0; }
int pg_ctx_vocab_get(pgorb_ctx* c, const uint8_t** d_blob, int* k, int* L, int* nnodes)
{
    if (!c->vocab.p || !c->vocabNodes) return fail(c, PGORB_E_ARG, "no vocabulary uploaded");
    *d_blob = (const uint8_t*)c->vocab.p; *k = c->vocabK; *L = c->vocabL; *nnodes = c->vocabNodes;
    return 0;
}
bool pg_ctx_vocab_kind(pgorb_ctx* c, int* scoring, int* weighting)
{
    if (!c->vocab.p || !c->vocabNodes) return false;
    *scoring = c->vocabScoring; *weighting = c->vocabWeighting;
    return true;
}

extern "C" {

int pgorb_create(const pgorb_params* p, pgorb_ctx** out)
{
    if (!p || !out) return fail(nullptr, PGORB_E_ARG, "null argument");
    *out = nullptr;
    if (p->nlevels < 1 || p->nlevels > PG_MAXL || p->nfeatures < 1 || !(p->scale_factor > 1.0f) ||
        p->max_batch < 1 || p->max_width < 62 || p->max_height < 62 || p->min_th_fast < 1 ||
        p->ini_th_fast < p->min_th_fast || p->ini_th_fast > 254)
        return fail(nullptr, PGORB_E_ARG, "invalid parameters");
    if (p->max_width > 4095 || p->max_height > 4095)
        return fail(nullptr, PGORB_E_LIMIT, "max_width/max_height above 4095 not supported");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev)
        return fail(nullptr, PGORB_E_NODEVICE, "no HIP device %d (found %d); libpgorb has no CPU path",
                    p->device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) != hipSuccess)
        return fail(nullptr, PGORB_E_NODEVICE, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PGORB_E_NODEVICE, "device %d is %s; libpgorb is built for gfx950 only",
                    p->device, prop.gcnArchName);
    if (hipSetDevice(p->device) != hipSuccess)
        return fail(nullptr, PGORB_E_HIP, "hipSetDevice failed");

    pgorb_ctx* c = new pgorb_ctx();
    c->prm = *p;
    c->mx = pg_match_default_opts();
    c->useGraph = getenv("PGORB_EXTRACT_NO_GRAPH") == nullptr;
    if (const char* e = getenv("PGORB_QT_THREADS")) { const int v = atoi(e); if (v == 256 || v == 512 || v == 1024) c->qtThreads = v; }
    if (const char* e = getenv("PGORB_QT_SPLIT")) { const int v = atoi(e); if (v >= 0 && v <= 2) c->qtSplit = v; }      // A / B switch of K3's two forms (option "quadtree_split")
    // ORBextractor.cc:415-446
    const int L = p->nlevels;
    c->scaleFactor = p->scale_factor;
    c->mvScaleFactor[0] = 1.0f; c->mvLevelSigma2[0] = 1.0f;
    for (int i = 1; i <= L; i++) {
        c->mvScaleFactor[i] = (float)(c->mvScaleFactor[i - 1] * c->scaleFactor);
        c->mvLevelSigma2[i] = c->mvScaleFactor[i] * c->mvScaleFactor[i];
    }
    for (int i = 0; i <= L; i++) {
        c->mvInvScaleFactor[i] = 1.0f / c->mvScaleFactor[i];
        c->mvInvLevelSigma2[i] = 1.0f / c->mvLevelSigma2[i];
    }
    const float factor = (float)(1.0f / c->scaleFactor);
    float nDesired = p->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L; l++) {
        c->mnFeaturesPerLevel[l] = (int)lrint((double)nDesired);      // cvRound
        sum += c->mnFeaturesPerLevel[l];
        nDesired *= factor;
    }
    c->mnFeaturesPerLevel[L] = std::max(p->nfeatures - sum, 0);
    *out = c;
    return 0;
}

void pgorb_destroy(pgorb_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->prm.device);
    while (!c->streams.empty()) pgorb_stream_destroy(c->streams.back());      // a stream holds a pointer to its context
    Arena* all[] = {&c->cellTab, &c->cellTabBal, &c->cellCand, &c->cellCount, &c->pyr, &c->cand, &c->sel, &c->nodes, &c->counters, &c->tables, &c->qtTab, &c->qtLeaf,
                    &c->outBlk, &c->stageA, &c->stageOut, &c->stageSfi, &c->vocab, &c->xdesc, &c->sim3Caps, &c->pnpTable};
    for (Arena* a : all) if (a->p) (void)hipFree(a->p);
    destroy_side_streams(c);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->hg.exec) (void)hipGraphExecDestroy(c->hg.exec);
    if (c->hg.g) (void)hipGraphDestroy(c->hg.g);
    if (c->sHost) { (void)hipStreamSynchronize(c->sHost); (void)hipStreamDestroy(c->sHost); }
    if (c->evSfi) (void)hipEventDestroy(c->evSfi);
    for (hipEvent_t e : c->evExtract) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->evMatch) (void)hipEventDestroy(e);
    delete c;
}

const char* pgorb_last_error(const pgorb_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int pgorb_levels(const pgorb_ctx* c) { return c ? c->prm.nlevels : PGORB_E_ARG; }

int pgorb_scale_tables(const pgorb_ctx* c, float* scale, float* inv, float* s2, float* is2)
{
    if (!c) return PGORB_E_ARG;
    const size_t n = (size_t)(c->prm.nlevels + 1) * sizeof(float);
    if (scale) memcpy(scale, c->mvScaleFactor, n);
    if (inv) memcpy(inv, c->mvInvScaleFactor, n);
    if (s2) memcpy(s2, c->mvLevelSigma2, n);
    if (is2) memcpy(is2, c->mvInvLevelSigma2, n);
    return 0;
}

int pgorb_features_per_level(const pgorb_ctx* c, int32_t* out)
{
    if (!c || !out) return PGORB_E_ARG;
    for (int i = 0; i <= c->prm.nlevels; i++) out[i] = c->mnFeaturesPerLevel[i];
    return 0;
}

int pgorb_max_keypoints(const pgorb_ctx* c, int w, int h)
{
    if (!c) return PGORB_E_ARG;
    if (w > c->prm.max_width || h > c->prm.max_height) return PGORB_E_LIMIT;
    LevelGeom g[PG_MAXL];
    int rc = level_geometry(c, w, h, g);
    if (rc) return rc;
    int total = 0;
    for (int l = 0; l < c->prm.nlevels; l++) total += std::max(c->mnFeaturesPerLevel[l] + 2, 4 * g[l].nIni);
    return total;
}

void* pgorb_host_alloc(int64_t bytes)
{
    void* p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void pgorb_host_free(void* p) { if (p) (void)hipHostFree(p); }

int pgorb_host_register(void* p, int64_t bytes)
{
    if (!p || bytes <= 0) return PGORB_E_ARG;
    if (hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return PGORB_E_HIP; }
    return PGORB_OK;
}

int pgorb_host_unregister(void* p)
{
    if (!p) return PGORB_E_ARG;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return PGORB_E_HIP; }
    return PGORB_OK;
}

int pgorb_descriptor_distance(const uint8_t* a, const uint8_t* b)
{
    if (!a || !b) return PGORB_E_ARG;
    int dist = 0;
    for (int i = 0; i < 32; i += 8) {
        uint64_t x, y;
        memcpy(&x, a + i, 8); memcpy(&y, b + i, 8);
        dist += __builtin_popcountll(x ^ y);
    }
    return dist;
}

int pgorb_hamming_matrix(pgorb_ctx* c, const uint8_t* a, int na, const uint8_t* b, int nb, uint16_t* out)
{
    if (!c) return PGORB_E_ARG;
    if (na < 0 || nb < 0 || (na && !a) || (nb && !b) || (na && nb && !out))
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_hamming_matrix");
    if (!na || !nb) return 0;
    PG_HIP(c, hipSetDevice(c->prm.device));
    // pageable copies, not PgHostCall: at 2000 x 2000 its page-locked download and host copy of the 8 MB matrix measured 531 us
    // per call on an MI355X, these 213 us
    const size_t offB = ((size_t)na * 32 + 63) & ~(size_t)63;
    int rc;
    if ((rc = ensure(c, c->stageA, offB + (size_t)nb * 32))) return rc;
    if ((rc = ensure(c, c->stageOut, (size_t)na * nb * 2))) return rc;
    uint8_t* dA = (uint8_t*)c->stageA.p;
    PG_HIP(c, hipMemcpy(dA, a, (size_t)na * 32, hipMemcpyHostToDevice));
    PG_HIP(c, hipMemcpy(dA + offB, b, (size_t)nb * 32, hipMemcpyHostToDevice));
    pg_launch_hamming_matrix(dA, na, dA + offB, nb, (uint16_t*)c->stageOut.p, 0);
    PG_HIP(c, hipGetLastError());
    PG_HIP(c, hipMemcpy(out, c->stageOut.p, (size_t)na * nb * 2, hipMemcpyDeviceToHost));
    return 0;
}

int pgorb_hamming_best2(pgorb_ctx* c, const uint8_t* a, int na, const uint8_t* b, int nb,
                        int32_t* best_idx, uint16_t* best, uint16_t* second)
{
    if (!c) return PGORB_E_ARG;
    if (na < 0 || nb < 0 || (na && (!a || !best_idx || !best || !second)) || (nb && !b))
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_hamming_best2");
    if (nb >= (1 << 20)) return fail(c, PGORB_E_LIMIT, "more than 2^20 train descriptors");
    if (!na) return 0;
    PG_HIP(c, hipSetDevice(c->prm.device));
    int rc;
    if ((rc = ensure(c, c->xdesc, pg_match_scratch_bytes(c->mx, nb, 1) + 16))) return rc;
    PgHostCall s(c);
    const size_t oA = s.region(PG_UP, (size_t)na * 32), oB = s.region(PG_UP, (size_t)nb * 32 + 32),
                 oI = s.region(PG_DOWN, (size_t)na * 4), oB1 = s.region(PG_DOWN, (size_t)na * 2), oB2 = s.region(PG_DOWN, (size_t)na * 2);
    if ((rc = s.begin())) return rc;
    s.put(oA, a, (size_t)na * 32); s.put(oB, b, (size_t)nb * 32, 0, (size_t)nb * 32 + 32);
    if ((rc = s.run([&] {
            pg_launch_best2(c->mx, s.dev(oA), na, s.dev(oB), nb, (uint8_t*)c->xdesc.p, s.dev<int32_t>(oI), s.dev<uint16_t>(oB1),
                            s.dev<uint16_t>(oB2), 0);
            PG_HIP(c, hipGetLastError());
            return 0; }))) return rc;
    memcpy(best_idx, s.host(oI), (size_t)na * 4);
    memcpy(best, s.host(oB1), (size_t)na * 2);
    memcpy(second, s.host(oB2), (size_t)na * 2);
    return 0;
}

int pgorb_match_batch_device(pgorb_ctx* c, const uint8_t* d_desc, const int32_t* d_n, int cap,
                             const int32_t* d_pq, const int32_t* d_pt, int npairs,
                             int32_t* d_best_idx, uint16_t* d_best, uint16_t* d_second, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_desc || !d_n || cap < 1 || npairs < 0 || (npairs && (!d_pq || !d_pt || !d_best_idx || !d_best || !d_second)))
        return fail(c, PGORB_E_ARG, "bad argument to pgorb_match_batch_device");
    PG_HIP(c, hipSetDevice(c->prm.device));
    if (cap >= (1 << 20)) return fail(c, PGORB_E_LIMIT, "more than 2^20 descriptors per frame");
    int rc;
    if ((rc = ensure(c, c->xdesc, pg_match_scratch_bytes(c->mx, cap, npairs) + 16))) return rc;
    hipEvent_t* ev = (c->profMatch < c->profMax) ? &c->evMatch[2 * (size_t)c->profMatch] : nullptr;
    if (ev) PG_HIP(c, hipEventRecord(ev[0], (hipStream_t)stream));
    pg_launch_match_batch(c->mx, d_desc, d_n, cap, d_pq, d_pt, npairs, (uint8_t*)c->xdesc.p, d_best_idx, d_best, d_second,
                          (hipStream_t)stream);
    if (ev) { PG_HIP(c, hipEventRecord(ev[1], (hipStream_t)stream)); c->profMatch++; }
    PG_HIP(c, hipGetLastError());
    return 0;
}

int pgorb_set_option(pgorb_ctx* c, const char* key, int value)
{
    if (!key) return PGORB_E_ARG;
    if (!c) return PGORB_E_ARG;                               // every option belongs to a context (round 4: no process-wide state)
    pg_forward_option_to_lanes(c, key, value);                // the sibling contexts of live multi-lane device streams follow
    c->planEpoch++;                                            // (a captured graph of the host-frame path holds the old settings)
    const PgOption* o = find_option(key);
    if (!o) return fail(c, PGORB_E_ARG, "unknown option '%s'", key);
    if (o->valid && !o->valid(value)) return fail(c, PGORB_E_ARG, "%s", o->error);
    o->at(c) = o->store ? o->store(value) : value;
    return 0;
}

int pgorb_get_option(const pgorb_ctx* c, const char* key)
{
    if (!key || !c) return PGORB_OPTION_UNKNOWN;
    if (!strcmp(key, "fused_launches")) return c->lastFusedLaunches;      // (read-only)
    const PgOption* o = find_option(key);
    return o ? o->at(const_cast<pgorb_ctx*>(c)) : PGORB_OPTION_UNKNOWN;
}

int pgorb_matcher_is_popcount(const pgorb_ctx* c, int cap_per_frame) { return pg_match_uses_popcount(c ? c->mx : pg_match_default_opts(), cap_per_frame) ? 1 : 0; }

}  // extern "C"
