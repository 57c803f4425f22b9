// frame.hip -- what Frame.cc does on gfx950: the keypoint grid, vbPrevMatched, undistortion and the image bounds.
//
// Restates (thirdparty/orb-slam2):
//   Frame::AssignFeaturesToGrid / PosInGrid   src/Frame.cc:234-249, 386-396
//   Frame::UndistortKeyPoints                 src/Frame.cc:398-437 (cv::undistortPoints)
//   Frame::ComputeImageBounds                 src/Frame.cc:439-467
// The matchers that read the grid are in init_match.hip, window_match.hip (GetFeaturesInArea's window: match_common.h) and fuse.hip.
#include "match_common.h"

__device__ __forceinline__ int grid_cell_of(const pgorb_keypoint& kp, float minX, float minY, float invW, float invH)
{
    const int posX = (int)roundf(__fmul_rn(__fsub_rn(kp.x, minX), invW));       // PosInGrid (:388-389)
    const int posY = (int)roundf(__fmul_rn(__fsub_rn(kp.y, minY), invH));
    return (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) ? -1 : posX * GRID_ROWS + posY;
}

__global__ __launch_bounds__(256) void k_frame_grid(const pgorb_keypoint* __restrict__ kps,
                                                     const int32_t* __restrict__ nper, int cap,
                                                     float minX, float minY, float invW, float invH,
                                                     int32_t* __restrict__ gstart, int32_t* __restrict__ gidx)
{
    __shared__ int cnt[GRID_CELLS];
    __shared__ int part[256 + 1];
    __shared__ int cellOf[256];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int n = min(nper[f], cap);
    const pgorb_keypoint* K = kps + (int64_t)f * cap;
    int32_t* start = gstart + (int64_t)f * (GRID_CELLS + 1);
    int32_t* idx = gidx + (int64_t)f * cap;
    for (int c = tid; c < GRID_CELLS; c += 256) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int c = grid_cell_of(K[i], minX, minY, invW, invH);
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan of the 3072 counters: 12 per thread
    {
        const int b = tid * 12;
        int sum = 0;
        for (int c = b; c < b + 12; c++) sum += cnt[c];
        // exclusive scan of the 256 partial sums: DPP scan inside each wave, the four wave totals by every thread (one thread walking
        // the 256 entries cost 14 of the kernel's 32 us)
        const int lane_ = tid & 63, wv_ = tid >> 6;
        const int incl = wave_incl_scan(sum, lane_);
        if (lane_ == 63) part[wv_] = incl;
        __syncthreads();
        int base_ = 0, total_ = 0;
        for (int w = 0; w < 4; w++) { const int v = part[w]; base_ += w < wv_ ? v : 0; total_ += v; }
        int run = base_ + incl - sum;
        if (tid == 255) part[256] = total_;
        for (int c = b; c < b + 12; c++) { const int v = cnt[c]; cnt[c] = run; start[c] = run; run += v; }
        if (tid == 255) start[GRID_CELLS] = total_;
    }
    __syncthreads();
    // stable placement: chunks of 256 keypoints in index order (mGrid[..].push_back(i), :246-247)
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const int c = (i < n) ? grid_cell_of(K[i], minX, minY, invW, invH) : -1;
        cellOf[tid] = c;
        __syncthreads();
        int pos = -1;
        if (c >= 0) {
            int rank = 0;
            for (int t = 0; t < tid; t++) rank += (cellOf[t] == c);
            pos = cnt[c] + rank;
        }
        __syncthreads();
        if (c >= 0) { atomicAdd(&cnt[c], 1); idx[pos] = i; }
        __syncthreads();
    }
}

// vbPrevMatched of MonocularInitialization: the reference frame's keypoint positions (Tracking.cc:583-585)
__global__ __launch_bounds__(256) void k_prev_matched_init(const pgorb_keypoint* __restrict__ kps, int64_t rows, float2* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) out[i] = make_float2(kps[i].x, kps[i].y);
}
void pg_launch_prev_matched_init(const pgorb_keypoint* d_kps, int64_t rows, float* d_out, hipStream_t s)
{
    if (rows > 0) hipLaunchKernelGGL(k_prev_matched_init, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_kps, rows, reinterpret_cast<float2*>(d_out));
}

// ---- cv::undistortPoints (OpenCV 2.4 imgproc/undistort.cpp cvUndistortPoints), 5 fixed-point
// iterations in double, R = identity, P = K.  Same operation order on host and device, no FMA.
struct PgCamera { double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3; };

__host__ __device__ inline void pg_undistort_point(const PgCamera& C, float px, float py, float* ox, float* oy)
{
#ifdef __HIP_DEVICE_COMPILE__
#define PGM(a, b) __dmul_rn((a), (b))
#define PGA(a, b) __dadd_rn((a), (b))
#define PGS(a, b) __dsub_rn((a), (b))
#define PGD(a, b) __ddiv_rn((a), (b))
#else
#define PGM(a, b) ((a) * (b))
#define PGA(a, b) ((a) + (b))
#define PGS(a, b) ((a) - (b))
#define PGD(a, b) ((a) / (b))
#endif
    double x = (double)px, y = (double)py;
    const double x0 = x = PGM(PGS(x, C.cx), C.ifx);
    const double y0 = y = PGM(PGS(y, C.cy), C.ify);
    for (int j = 0; j < 5; j++) {
        const double r2 = PGA(PGM(x, x), PGM(y, y));
        // icdist = (1 + ((k[7]*r2 + k[6])*r2 + k[5])*r2) / (1 + ((k[4]*r2 + k[1])*r2 + k[0])*r2), k5..k7 = 0
        const double icdist = PGD(1.0, PGA(1.0, PGM(PGA(PGM(PGA(PGM(C.k3, r2), C.k2), r2), C.k1), r2)));
        const double deltaX = PGA(PGM(PGM(PGM(2.0, C.p1), x), y), PGM(C.p2, PGA(r2, PGM(PGM(2.0, x), x))));
        const double deltaY = PGA(PGM(C.p1, PGA(r2, PGM(PGM(2.0, y), y))), PGM(PGM(PGM(2.0, C.p2), x), y));
        x = PGM(PGS(x0, deltaX), icdist);
        y = PGM(PGS(y0, deltaY), icdist);
    }
    // RR = P * R = K: xx = fx*x + 0*y + cx, ww = 1/(0*x + 0*y + 1)
    const double xx = PGA(PGA(PGM(C.fx, x), PGM(0.0, y)), C.cx);
    const double yy = PGA(PGA(PGM(0.0, x), PGM(C.fy, y)), C.cy);
    const double ww = PGD(1.0, PGA(PGA(PGM(0.0, x), PGM(0.0, y)), 1.0));
    *ox = (float)PGM(xx, ww);
    *oy = (float)PGM(yy, ww);
#undef PGM
#undef PGA
#undef PGS
#undef PGD
}

static PgCamera pg_make_camera(const float camera[4], const float dist[5])
{
    PgCamera C;
    C.fx = camera[0]; C.fy = camera[1]; C.cx = camera[2]; C.cy = camera[3];
    C.ifx = 1. / C.fx; C.ify = 1. / C.fy;
    C.k1 = dist[0]; C.k2 = dist[1]; C.p1 = dist[2]; C.p2 = dist[3]; C.k3 = dist[4];
    return C;
}

__global__ __launch_bounds__(256) void k_undistort_keypoints(const pgorb_keypoint* __restrict__ in,
                                                              const int32_t* __restrict__ nper, int cap,
                                                              PgCamera C, int identity, pgorb_keypoint* __restrict__ out)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(nper[f], cap)) return;
    pgorb_keypoint k = in[(int64_t)f * cap + i];
    if (!identity) pg_undistort_point(C, k.x, k.y, &k.x, &k.y);
    out[(int64_t)f * cap + i] = k;
}

extern "C" {

int pgorb_undistort_keypoints_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes,
                                           int cap, const float camera[4], const float dist[5], pgorb_keypoint* d_out,
                                           void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || !d_out || nframes < 1 || cap < 1 || !camera || !dist)
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_undistort_keypoints_batch_device");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    hipLaunchKernelGGL(k_undistort_keypoints, dim3((cap + 255) / 256, nframes), dim3(256), 0, (hipStream_t)stream, d_kps, d_n,
                       cap, pg_make_camera(camera, dist), dist[0] == 0.0f ? 1 : 0, d_out);      // Frame.cc:410
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_undistort_keypoints launch failed");
    return 0;
}

int pgorb_undistort_keypoints(pgorb_ctx* c, const pgorb_keypoint* kps, int n, const float camera[4], const float dist[5],
                              pgorb_keypoint* out)
{
    if (!c) return PGORB_E_ARG;
    if (n < 0 || (n && (!kps || !out)) || !camera || !dist) return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_undistort_keypoints");
    if (!n) return 0;
    const size_t kb = (size_t)n * sizeof(pgorb_keypoint);
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 4), oK = s.region(PG_UP, kb), oOut = s.region(PG_DOWN, kb);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, &n, 4); s.put(oK, kps, kb);
    if ((rc = s.run([&] { return pgorb_undistort_keypoints_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), 1, n, camera, dist,
                                                                        s.dev<pgorb_keypoint>(oOut), nullptr); }))) return rc;
    memcpy(out, s.host(oOut), kb);
    return 0;
}

int pgorb_image_bounds(int cols, int rows, const float camera[4], const float dist[5], float bounds[4])
{
    if (cols < 1 || rows < 1 || !camera || !dist || !bounds) return PGORB_E_ARG;
    if (dist[0] == 0.0f) {                                     // Frame.cc:461-466
        bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows;
        return 0;
    }
    const PgCamera C = pg_make_camera(camera, dist);
    const float cx[4] = {0.0f, (float)cols, 0.0f, (float)cols}, cy[4] = {0.0f, 0.0f, (float)rows, (float)rows};
    float ux[4], uy[4];
    for (int i = 0; i < 4; i++) pg_undistort_point(C, cx[i], cy[i], &ux[i], &uy[i]);
    bounds[0] = std::min(ux[0], ux[2]); bounds[1] = std::max(ux[1], ux[3]);     // Frame.cc:455-458
    bounds[2] = std::min(uy[0], uy[1]); bounds[3] = std::max(uy[2], uy[3]);
    return 0;
}

int pgorb_frame_grid(pgorb_ctx* c, const pgorb_keypoint* kps, int n, float min_x, float max_x, float min_y,
                     float max_y, int32_t* grid_start, int32_t* grid_idx)
{
    if (!c) return PGORB_E_ARG;
    if (n < 0 || (n && (!kps || !grid_idx)) || !grid_start) return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_frame_grid");
    const int cap = n > 0 ? n : 1;
    PgHostCall s(c);
    const size_t oN = s.region(PG_UP, 4), oK = s.region(PG_UP, (size_t)cap * sizeof(pgorb_keypoint)),
                 oS = s.region(PG_DOWN, (size_t)(GRID_CELLS + 1) * 4), oI = s.region(PG_DOWN, (size_t)cap * 4);
    int rc = s.begin();
    if (rc) return rc;
    s.put(oN, &n, 4); s.put(oK, kps, (size_t)n * sizeof(pgorb_keypoint));
    if ((rc = s.run([&] { return pgorb_frame_grid_batch_device(c, s.dev<pgorb_keypoint>(oK), s.dev<int32_t>(oN), 1, cap, min_x, max_x, min_y,
                                                               max_y, s.dev<int32_t>(oS), s.dev<int32_t>(oI), nullptr); }))) return rc;
    memcpy(grid_start, s.host(oS), (size_t)(GRID_CELLS + 1) * 4);
    if (n) memcpy(grid_idx, s.host(oI), (size_t)n * 4);
    return 0;
}

int pgorb_frame_grid_batch_device(pgorb_ctx* c, const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes,
                                  int cap, float min_x, float max_x, float min_y, float max_y,
                                  int32_t* d_grid_start, int32_t* d_grid_idx, void* stream)
{
    if (!c) return PGORB_E_ARG;
    if (!d_kps || !d_n || nframes < 1 || cap < 1 || !d_grid_start || !d_grid_idx || !(max_x > min_x) || !(max_y > min_y))
        return pg_ctx_fail(c, PGORB_E_ARG, "bad argument to pgorb_frame_grid_batch_device");
    if (hipSetDevice(pg_ctx_device(c)) != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "hipSetDevice failed");
    const float invW = (float)GRID_COLS / (max_x - min_x), invH = (float)GRID_ROWS / (max_y - min_y);   // Frame.cc:216-217
    hipLaunchKernelGGL(k_frame_grid, dim3(nframes), dim3(256), 0, (hipStream_t)stream, d_kps, d_n, cap, min_x, min_y,
                       invW, invH, d_grid_start, d_grid_idx);
    if (hipGetLastError() != hipSuccess) return pg_ctx_fail(c, PGORB_E_HIP, "k_frame_grid launch failed");
    return 0;
}

}  // extern "C"
