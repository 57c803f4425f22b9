/* include/pgorb.h -- C ABI of libpgorb.so, the MI355X (gfx950) ORB front end.
 *
 * Drop-in boundary for pilotguru's per-frame visual-odometry front end.  The
 * reference has no FFI layer; its seam is a C++ functor plus two helpers
 * (SURVEY.md section 8b).  Each entry point below names the reference
 * interface it replaces (paths relative to the reference tree):
 *
 *   pgorb_create / pgorb_destroy     ORBextractor::ORBextractor(nfeatures, scaleFactor,
 *                                    nlevels, iniThFAST, minThFAST)
 *                                    thirdparty/orb-slam2/include/ORBextractor.h:51-54,
 *                                    constructed at src/Tracking.cc:137-143
 *   pgorb_extract*                   ORBextractor::operator()(image, mask, keypoints,
 *                                    descriptors)  include/ORBextractor.h:59-61,
 *                                    called from Frame::ExtractORB src/Frame.cc:251-257
 *   pgorb_scale_tables, _levels      GetScaleFactors()/GetInverseScaleFactors()/
 *                                    GetScaleSigmaSquares()/GetInverseScaleSigmaSquares()/
 *                                    GetLevels()  include/ORBextractor.h:63-83
 *   pgorb_descriptor_distance        static ORBmatcher::DescriptorDistance(a, b)
 *                                    include/ORBmatcher.h:44, src/ORBmatcher.cc:1651-1667
 *   pgorb_hamming_*                  the candidate-scan inner loops of the matchers
 *                                    (src/ORBmatcher.cc:438-459 etc.) as an all-pairs
 *                                    superset
 *
 * Conventions: plain pointers and sizes, caller owns every buffer, integer
 * status codes (0 = ok, <0 = error, text via pgorb_last_error) instead of the
 * reference's assert()/silent return (src/ORBextractor.cc:1045-1049).  One
 * context per host thread and device, like the reference's non-re-entrant
 * extractor.  There is NO CPU fallback: without a HIP device pgorb_create
 * fails with PGORB_E_NODEVICE.
 *
 * "_device" entry points take device pointers and a hipStream_t (passed as
 * void*) and are asynchronous on that stream; the others take host pointers
 * and are synchronous.
 */
#ifndef PGORB_H
#define PGORB_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PGORB_MAX_LEVELS 16

enum {
    PGORB_OK = 0,
    PGORB_E_ARG = -1,        /* bad argument                                            */
    PGORB_E_TOOSMALL = -2,   /* a pyramid level has no 30-px cell (the reference divides
                                by zero there) or aspect < 0.5 (DistributeOctTree nIni=0) */
    PGORB_E_CAP = -3,        /* output capacity too small; nothing truncated silently   */
    PGORB_E_NODEVICE = -4,   /* no HIP device / wrong architecture                      */
    PGORB_E_HIP = -5,        /* HIP runtime error (see pgorb_last_error)                */
    PGORB_E_LIMIT = -6,      /* exceeds max_width/max_height/max_batch of the context, a
                              * level larger than 4095 px a side, more than 65533 keypoints
                              * on one level (the level's share of nfeatures), or a size
                              * limit stated at the call (DESIGN.md section 7 lists all)   */
    PGORB_E_OVERFLOW = -7    /* internal candidate capacity exceeded                    */
};

typedef struct pgorb_ctx pgorb_ctx;

typedef struct pgorb_params {
    int32_t nfeatures;       /* ORBextractor_nFeatures  (src/Tracking.cc:131)            */
    float   scale_factor;    /* ORBextractor_scaleFactor                                 */
    int32_t nlevels;         /* ORBextractor_nLevels, 1..PGORB_MAX_LEVELS                */
    int32_t ini_th_fast;     /* ORBextractor_iniThFAST                                   */
    int32_t min_th_fast;     /* ORBextractor_minThFAST                                   */
    int32_t max_width;       /* largest frame the context must hold (<= 4095)            */
    int32_t max_height;
    int32_t max_batch;       /* frames per pgorb_extract_batch* call                     */
    int32_t device;          /* HIP device ordinal                                       */
    int32_t blur_tie_mode;   /* 0: OpenCV x86-64 binary rounding of the blur column pass
                                (ties to even for x < (w & ~3)); 1: half-up everywhere   */
} pgorb_params;

/* == cv::KeyPoint of OpenCV 2.4 (pt.x, pt.y, size, angle, response, octave, class_id) */
typedef struct pgorb_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} pgorb_keypoint;

int  pgorb_create(const pgorb_params* params, pgorb_ctx** out);
void pgorb_destroy(pgorb_ctx* ctx);
/* Last error text of `ctx` (or of the failed pgorb_create when ctx == NULL). */
const char* pgorb_last_error(const pgorb_ctx* ctx);

int  pgorb_levels(const pgorb_ctx* ctx);
/* nlevels+1 entries each (the reference sizes its tables nlevels+1, ORBextractor.cc:415-433);
 * any pointer may be NULL. */
int  pgorb_scale_tables(const pgorb_ctx* ctx, float* scale, float* inv_scale,
                        float* sigma2, float* inv_sigma2);
/* nlevels+1 entries (last = the fork's unused remainder slot, ORBextractor.cc:446) */
int  pgorb_features_per_level(const pgorb_ctx* ctx, int32_t* out);
/* Keypoint capacity that a w x h frame can never exceed: sum over levels of
 * max(quota + 2, 4 * nIni) (DistributeOctTree may overshoot its quota by up to 2 when the
 * last split adds 3 nodes, ORBextractor.cc:730; nIni = initial nodes, :543).
 * <0 when the frame is unusable (PGORB_E_TOOSMALL / PGORB_E_LIMIT). */
int  pgorb_max_keypoints(const pgorb_ctx* ctx, int w, int h);

/* Page-locked host memory for frames / results: host-buffer entry points run at PCIe speed when
 * their buffers come from here (pageable memory is staged by the driver at a fraction of it). */
void* pgorb_host_alloc(int64_t bytes);
void  pgorb_host_free(void* p);
/* Page-lock memory the CALLER owns (a frame buffer a decoder reuses call after call, e.g. the cv::Mat behind
 * Frame.cc:251-257): pgorb_extract* then uploads it with ONE DMA instead of copying it through the library's staging
 * slot (the host thread's 2 MB memcpy per 1080p frame).  The caller keeps the obligation the ownership implies:
 * pgorb_host_unregister before the memory is freed or remapped -- which is why the library does not do this behind
 * the caller's back, keyed by address.  Returns PGORB_OK, PGORB_E_ARG, or PGORB_E_HIP (the range cannot be locked). */
int   pgorb_host_register(void* p, int64_t bytes);
int   pgorb_host_unregister(void* p);

/* One frame, host buffers.  gray: h rows of `stride` bytes.  kps[cap], desc[cap*32]. */
int  pgorb_extract(pgorb_ctx* ctx, const uint8_t* gray, int w, int h, int stride,
                   pgorb_keypoint* kps, uint8_t* desc, int cap, int* n);
/* nframes frames of equal size, host buffers; frame f writes kps[f*cap_per_frame ...],
 * desc[(f*cap_per_frame)*32 ...], n[f]. */
int  pgorb_extract_batch(pgorb_ctx* ctx, const uint8_t* const* gray, int nframes,
                         int w, int h, int stride,
                         pgorb_keypoint* kps, uint8_t* desc, int cap_per_frame, int* n);
/* Same, everything resident in HBM: d_gray = nframes planes `frame_stride` bytes apart.
 * Asynchronous on `hip_stream`.  d_n[f] receives the true count even when it exceeds
 * cap_per_frame (then only the first cap_per_frame entries were written).
 * Level 0 aliases d_gray when d_gray, stride and frame_stride are multiples of 4.  Only bytes
 * 0 .. w-1 of each row decide the results: the bytes between w and `stride`, and between
 * frames, may hold anything, and rows other than a frame's last may be read up to `stride`.
 * Of a frame's last row no byte past the w-th is read (the pyramid's first resize and the
 * fused launch copy such chunks byte by byte), so the allocation may end there (a crop, or
 * buf[..., :w] at the end of a tensor). */
int  pgorb_extract_batch_device(pgorb_ctx* ctx, const uint8_t* d_gray, int nframes,
                                int w, int h, int stride, int64_t frame_stride,
                                pgorb_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame,
                                int32_t* d_n, void* hip_stream);
/* Colour ingest: Tracking::GrabImageMonocular's cvtColor (src/Tracking.cc:247-260) fused in
 * front of the extractor.  d_img = nframes interleaved 8-bit images with `channels` = 3 or 4
 * bytes per pixel, rgb_order != 0 for R,G,B(,A) (Camera_RGB: 1), 0 for B,G,R(,A).
 * gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (OpenCV 2.4 CV_RGB2GRAY, 8U).  The grey
 * planes are written straight into the context's pyramid level 0. */
int  pgorb_extract_batch_color_device(pgorb_ctx* ctx, const uint8_t* d_img, int nframes,
                                      int w, int h, int stride, int64_t frame_stride,
                                      int channels, int rgb_order,
                                      pgorb_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame,
                                      int32_t* d_n, void* hip_stream);
/* The reader's geometry as well: frames exactly as decoded, upright frames into the extractor.
 * rotate_degrees in {0, 90, 180, 270} as the video metadata says (src/io/image_sequence_reader.cc:
 * 186-205: 90 = cv::flip(raw.t(), 0), 180 = cv::flip(raw, -1), 270 = cv::flip(raw.t(), 1)), then
 * the optional --vertical_flip / --horizontal_flip of the wrapper source (:53-58, :212-222;
 * src/optical_trajectories.cc:49-52,84-85), then Tracking's grey conversion as above
 * (channels = 1: already grey).  Extracted frames are src_h x src_w for 90 / 270. */
int  pgorb_extract_batch_ingest_device(pgorb_ctx* ctx, const uint8_t* d_img, int nframes,
                                       int src_w, int src_h, int stride, int64_t frame_stride,
                                       int channels, int rgb_order, int rotate_degrees,
                                       int vertical_flip, int horizontal_flip,
                                       pgorb_keypoint* d_kps, uint8_t* d_desc, int cap_per_frame,
                                       int32_t* d_n, void* hip_stream);

/* Device status word of the last *_device call: 0 or PGORB_E_OVERFLOW.  Synchronises. */
int  pgorb_check_async(pgorb_ctx* ctx, void* hip_stream);

/* ORBmatcher::DescriptorDistance on two 32-byte descriptors (host, no device work). */
int  pgorb_descriptor_distance(const uint8_t* a, const uint8_t* b);
/* All-pairs Hamming: out[i*nb + j] = distance(a[i], b[j]).  Host buffers. */
int  pgorb_hamming_matrix(pgorb_ctx* ctx, const uint8_t* a, int na, const uint8_t* b, int nb,
                          uint16_t* out);
/* Best and second-best train descriptor per query (first minimum wins, strict <, like
 * the bestDist/bestDist2 scans in src/ORBmatcher.cc:438-459).  best_idx = -1 and
 * best = second = 65535 when nb == 0; second = 65535 when nb == 1.  PGORB_E_LIMIT for nb >= 2^20 (the popcount
 * kernel's key is distance << 20 | train index); the batched form below refuses cap_per_frame >= 2^20 likewise. */
int  pgorb_hamming_best2(pgorb_ctx* ctx, const uint8_t* a, int na, const uint8_t* b, int nb,
                         int32_t* best_idx, uint16_t* best, uint16_t* second);
/* Batched, resident: pair p matches descriptors of frame qa[p] (queries) against frame
 * qb[p] (train) inside one extract batch layout (desc base + f*cap_per_frame*32, counts
 * d_n[f] clamped to cap_per_frame).  Outputs are [npairs][cap_per_frame]. */
int  pgorb_match_batch_device(pgorb_ctx* ctx, const uint8_t* d_desc, const int32_t* d_n,
                              int cap_per_frame, const int32_t* d_pair_query,
                              const int32_t* d_pair_train, int npairs,
                              int32_t* d_best_idx, uint16_t* d_best, uint16_t* d_second,
                              void* hip_stream);

/* ---- Frame grid + guided matcher for initialisation ---------------------------------------
 *   pgorb_frame_grid*            Frame::AssignFeaturesToGrid / PosInGrid
 *                                thirdparty/orb-slam2/src/Frame.cc:234-249, 386-396 (64 x 48 grid,
 *                                include/Frame.h:37-38) as CSR: cell = col*48 + row,
 *                                start[3073], idx[] in insertion (= keypoint) order
 *   pgorb_search_for_initialization*   ORBmatcher::SearchForInitialization(F1, F2,
 *                                vbPrevMatched, vnMatches12, windowSize)
 *                                src/ORBmatcher.cc:407-522 incl. GetFeaturesInArea
 *                                (Frame.cc:331-384), TH_LOW = 50, the nnratio test, the
 *                                30-bin rotation histogram and ComputeThreeMaxima (:1605-1646)
 * Keypoints are taken as already undistorted (pilotguru calibrations with k1 == 0 skip
 * cv::undistortPoints, Frame.cc:410-414) and the bounds are the image rectangle
 * (Frame.cc:461-466): pass min_x = 0, max_x = cols, min_y = 0, max_y = rows.
 * The batched device forms work on the layout of pgorb_extract_batch_device. */
/*   pgorb_undistort_keypoints*   Frame::UndistortKeyPoints (src/Frame.cc:408-438) =
 *       cv::undistortPoints(pts, pts, mK, mDistCoef, Mat(), mK): camera = {fx, fy, cx, cy},
 *       dist = {k1, k2, p1, p2, k3} (as float, like mK / mDistCoef).  k1 == 0 copies the
 *       keypoints unchanged (:410-414).  Only pt.x / pt.y change.
 *   pgorb_image_bounds           Frame::ComputeImageBounds (src/Frame.cc:440-467): bounds =
 *       {mnMinX, mnMaxX, mnMinY, mnMaxY} from the four undistorted image corners. */
int  pgorb_undistort_keypoints(pgorb_ctx* ctx, const pgorb_keypoint* kps, int n,
                               const float camera[4], const float dist[5], pgorb_keypoint* out);
int  pgorb_undistort_keypoints_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps,
                               const int32_t* d_n, int nframes, int cap_per_frame,
                               const float camera[4], const float dist[5],
                               pgorb_keypoint* d_out, void* hip_stream);
int  pgorb_image_bounds(int cols, int rows, const float camera[4], const float dist[5], float bounds[4]);
#define PGORB_GRID_COLS 64
#define PGORB_GRID_ROWS 48
#define PGORB_GRID_CELLS (PGORB_GRID_COLS * PGORB_GRID_ROWS)
int  pgorb_frame_grid(pgorb_ctx* ctx, const pgorb_keypoint* kps, int n,
                      float min_x, float max_x, float min_y, float max_y,
                      int32_t* grid_start /*[3073]*/, int32_t* grid_idx /*[n]*/);
int  pgorb_frame_grid_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n,
                                   int nframes, int cap_per_frame,
                                   float min_x, float max_x, float min_y, float max_y,
                                   int32_t* d_grid_start /*[nframes][3073]*/,
                                   int32_t* d_grid_idx /*[nframes][cap]*/, void* hip_stream);
/* prev_matched: float[2*n1] in/out (vbPrevMatched); matches12: int32[n1] out (-1 = none);
 * returns nmatches (>= 0) or an error code.  PGORB_E_LIMIT above 16000 keypoints in either frame (cap_per_frame in the batched
 * form); the grid calls above have no limit of their own. */
int  pgorb_search_for_initialization(pgorb_ctx* ctx,
                                     const pgorb_keypoint* kps1, const uint8_t* desc1, int n1,
                                     const pgorb_keypoint* kps2, const uint8_t* desc2, int n2,
                                     float min_x, float max_x, float min_y, float max_y,
                                     float* prev_matched, int32_t* matches12,
                                     int window_size, float nnratio, int check_orientation);
/* pair p: F1 = frame pair_f1[p], F2 = frame pair_f2[p]; d_prev_matched / d_matches12 are
 * [npairs][cap]; d_nmatches[npairs]. */
int  pgorb_search_for_initialization_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps,
                                     const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
                                     const int32_t* d_grid_start, const int32_t* d_grid_idx,
                                     const int32_t* d_pair_f1, const int32_t* d_pair_f2, int npairs,
                                     float min_x, float max_x, float min_y, float max_y,
                                     float* d_prev_matched, int32_t* d_matches12, int32_t* d_nmatches,
                                     int window_size, float nnratio, int check_orientation,
                                     void* hip_stream);

/* ---- Guided matchers of the tracking thread (next tier of SURVEY.md 8a row a11) -------------
 *   pgorb_search_by_projection_points   ORBmatcher::SearchByProjection(Frame &F, const
 *       vector<MapPoint*> &vpMapPoints, float th)  src/ORBmatcher.cc:46-131 incl.
 *       RadiusByViewingCos :133-139 -- the local-map matcher of Tracking::SearchLocalPoints
 *       (src/Tracking.cc:1134-1184).  Per map point the caller passes what MapPoint carries after
 *       Frame::isInFrustum: mbTrackInView && !isBad() (valid), mTrackProjX/Y, mnTrackScaleLevel,
 *       mTrackViewCos, GetDescriptor(), Observations() > 0.
 *   pgorb_search_by_projection_frame    the matching loop of ORBmatcher::SearchByProjection(Frame
 *       &CurrentFrame, const Frame &LastFrame, float th, bool bMono)  src/ORBmatcher.cc:1355-1474
 *       for bMono = true, given the projections (u, v) of the last frame's map points into the
 *       current frame (the cv::Mat pose arithmetic of :1343-1377 stays with the caller, who owns
 *       the poses): valid = has a map point && !outlier && invzc >= 0 && inside the image
 *       bounds; octave/angle of the last frame's keypoint; best match only, TH_HIGH, rotation
 *       histogram + ComputeThreeMaxima.
 * Common state: kp_has_point[i] != 0 when the frame's keypoint i already holds a map point with
 * Observations() > 0 before the call (:79-81 / :1397-1399); assigned[i] receives the index of the
 * query (map point) written to F.mvpMapPoints[i] by this call, or -1.  Queries are processed in
 * order (each assignment changes what later queries may take): the results equal the reference's
 * sequence; since round 4 the device decides provably independent queries together.
 * Limits (all three forms, single and batched; PGORB_E_LIMIT): the deciding kernel keeps keypoints and queries in LDS, so what
 * bounds a call is  keypoints * 13 + queries * 10 + 256 <= 163840 bytes  (n and the number of queries in a single call,
 * cap_per_frame and qcap in a batched one), and 16000 for each count alone: 12582 keypoints with one query, 7112 with 7112
 * queries, 1000 with 15058.  Split the query list to match a larger frame. */
int  pgorb_search_by_projection_points(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n,            /* the frame F             */
        float min_x, float max_x, float min_y, float max_y,
        const uint8_t* kp_has_point,                                      /* [n]                     */
        int npoints, const uint8_t* valid, const float* proj_x, const float* proj_y,
        const int32_t* level, const float* view_cos, const uint8_t* point_desc,
        const uint8_t* point_has_obs, float th, float nnratio,
        int32_t* assigned /*[n]*/);                                       /* returns nmatches        */
int  pgorb_search_by_projection_frame(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n,            /* CurrentFrame            */
        float min_x, float max_x, float min_y, float max_y,
        const uint8_t* kp_has_point,
        int nlast, const uint8_t* valid, const float* u, const float* v,
        const int32_t* last_octave, const float* last_angle, const uint8_t* point_desc,
        const uint8_t* point_has_obs, float th, int check_orientation,
        int32_t* assigned /*[n]*/);                                       /* returns nmatches        */

/*   pgorb_search_by_projection_keyframe   the matching loop of ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF,
 *       const set<MapPoint*> &sAlreadyFound, float th, int ORBdist)  src/ORBmatcher.cc:1476-1603 -- the projection search of
 *       Tracking::Relocalization (src/Tracking.cc:1434: th 10, ORBdist 100; :1448: th 3, ORBdist 64).  Per map point i of the
 *       key frame the caller passes what its pose arithmetic (:1497-1517, cv::Mat) produced: valid = pMP && !pMP->isBad();
 *       already_found = sAlreadyFound.count(pMP); (u, v) the projection into the current frame; dist3d = |x3Dw - Ow|;
 *       min / max_distance = the point's mfMinDistance / mfMaxDistance (NOT the *Invariance() getters);
 *       kf_angle = pKF->mvKeysUn[i].angle; GetDescriptor().
 *       The device does the rest: the image-bounds test (:1512-1515), the depth-range test against
 *       GetMin/MaxDistanceInvariance() = 0.8f * min_distance / 1.2f * max_distance (:1519-1526, src/MapPoint.cc:390-400),
 *       MapPoint::PredictScale on the plain max_distance (src/MapPoint.cc:516-531) with log_scale_factor = CurrentFrame.mfLogScaleFactor, radius th * mvScaleFactors[level],
 *       levels level - 1 .. level + 1, best match only with ORBdist, rotation histogram.  Here ANY point in
 *       CurrentFrame.mvpMapPoints[i2] blocks a keypoint (:1542-1543: no Observations() test): kp_has_point[i2] != 0.
 *       PredictScale's `log` is the platform's logf in the reference; here a fixed double-precision sequence rounded once
 *       (pgorb_log_f; DESIGN.md section 5, parity contract 5), and pgorb_log_scale_factor is mfLogScaleFactor under it. */
int  pgorb_search_by_projection_keyframe(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n,            /* CurrentFrame            */
        float min_x, float max_x, float min_y, float max_y,
        const uint8_t* kp_has_point,
        int npoints, const uint8_t* valid, const uint8_t* already_found, const float* u, const float* v,
        const float* dist3d, const float* min_distance, const float* max_distance,
        const float* kf_angle, const uint8_t* point_desc,
        float log_scale_factor, float th, int orb_dist, int check_orientation,
        int32_t* assigned /*[n]*/);                                       /* returns nmatches        */
float pgorb_log_f(float x);
float pgorb_log_scale_factor(const pgorb_ctx* ctx);                      /* Frame::mfLogScaleFactor (Frame.cc:188)     */
int   pgorb_predict_scale(const pgorb_ctx* ctx, float max_distance, float current_dist);   /* MapPoint::PredictScale */

/*   pgorb_search_by_bow   ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*>
 *       &vpMapPointMatches)  src/ORBmatcher.cc:161-290 (Tracking::TrackReferenceKeyFrame,
 *       src/Tracking.cc:758; relocalisation :1359).  Both FeatureVectors come as the CSR arrays
 *       pgorb_bow_vectors produces (ascending node ids).  kf_point_valid[i] = the key frame's
 *       keypoint i has a map point that is not bad.  matches[j] = key-frame keypoint index whose
 *       map point was written to vpMapPointMatches[j], or -1.  Returns nmatches.  PGORB_E_LIMIT above 16000 features in
 *       either frame. */
int  pgorb_search_by_bow(pgorb_ctx* ctx,
        const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_point_valid, int nkf,
        const uint32_t* kf_fv_node, const int32_t* kf_fv_start, const uint32_t* kf_fv_feat, int kf_nfv,
        const uint8_t* f_desc, const float* f_angle, int nf,
        const uint32_t* f_fv_node, const int32_t* f_fv_start, const uint32_t* f_fv_feat, int f_nfv,
        float nnratio, int check_orientation, int32_t* matches /*[nf]*/);

/* Batched, resident forms of the three matchers above (round 3; the single calls are one-pair batches of these).
 * Frames live in the layout of pgorb_extract_batch_device (keypoints / descriptors `cap_per_frame` apart, counts d_n),
 * grids as pgorb_frame_grid_batch_device writes them; pair p matches its queries against frame d_pair_frame[p]
 * (NULL: frame p).  Query arrays are [npairs][qcap] with d_nq[p] entries in use; d_kp_has_point (NULL = none) and
 * d_assigned are [npairs][cap_per_frame], d_nmatches [npairs].  The reference's order dependence (an assignment is seen
 * by every later query, ORBmatcher.cc:75-79, :1398-1402, :236-240) stays inside a pair; pairs run concurrently.  SearchByProjection:
 * two passes (candidates and distances of every query in parallel; then one workgroup per pair decides the queries in rounds
 * of independent ones, every decision equal to the reference's sequence -- round 4);
 * SearchByBoW: one wave per common vocabulary node (a frame feature belongs to one node, so nodes are independent).  Call sites: Tracking::SearchLocalPoints (Tracking.cc:1175), TrackWithMotionModel (:876, :882),
 * TrackReferenceKeyFrame (:758). */
int  pgorb_search_by_projection_points_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point,
        int qcap, const int32_t* d_nq, const uint8_t* d_valid, const float* d_proj_x, const float* d_proj_y,
        const int32_t* d_level, const float* d_view_cos, const uint8_t* d_point_desc, const uint8_t* d_point_has_obs,
        float th, float nnratio, int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);
int  pgorb_search_by_projection_frame_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point,
        int qcap, const int32_t* d_nq, const uint8_t* d_valid, const float* d_u, const float* d_v,
        const int32_t* d_last_octave, const float* d_last_angle, const uint8_t* d_point_desc, const uint8_t* d_point_has_obs,
        float th, int check_orientation, int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);
int  pgorb_search_by_projection_keyframe_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const uint8_t* d_kp_has_point,
        int qcap, const int32_t* d_nq, const uint8_t* d_valid, const uint8_t* d_already_found, const float* d_u, const float* d_v,
        const float* d_dist3d, const float* d_min_distance, const float* d_max_distance, const float* d_kf_angle,
        const uint8_t* d_point_desc, float log_scale_factor, float th, int orb_dist, int check_orientation,
        int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);
/* FeatureVector of every frame on the device: from the per-feature node ids pgorb_bow_transform_device wrote
 * (d_node [nframes][cap]) the CSR arrays of DBoW2's FeatureVector (FeatureVector.cpp:31-45: node ids ascending,
 * feature indices of a node in feature order): d_fv_node / d_fv_feat [nframes][cap], d_fv_start [nframes][cap + 1],
 * d_nfv [nframes].  Equal to what pgorb_bow_vectors returns as fv_node / fv_start / fv_feat. */
int  pgorb_feature_vectors_batch_device(pgorb_ctx* ctx, const uint32_t* d_node, const int32_t* d_n, int nframes, int cap_per_frame,
        uint32_t* d_fv_node, int32_t* d_fv_start, uint32_t* d_fv_feat, int32_t* d_nfv, void* hip_stream);
/* pair p: key frame d_pair_kf[p], frame d_pair_f[p] of the same batch; d_kf_point_valid and d_matches [npairs][cap]. */
int  pgorb_search_by_bow_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
        const int32_t* d_pair_kf, const int32_t* d_pair_f, int npairs, const uint8_t* d_kf_point_valid,
        float nnratio, int check_orientation, int32_t* d_matches, int32_t* d_nmatches, void* hip_stream);

/* ---- The tracking thread's projection matchers with the projection on the device (csrc/track.hip) ---------------------------
 * The three pgorb_search_by_projection_* calls above take the projections as inputs; these three take what the rest of the
 * library takes -- poses, the resident map-point table of pgorb_fuse and table indices -- and run the front part on the device too:
 *   pgorb_search_local_points                  Tracking::SearchLocalPoints (src/Tracking.cc:1134-1184) from its first loop to the
 *       matcher's return, with Frame::isInFrustum (src/Frame.cc:273-329) and SearchByProjection(F, points, th) (ORBmatcher.cc:46-131);
 *   pgorb_search_by_projection_last_frame      all of SearchByProjection(CurrentFrame, LastFrame, th, bMono = true)
 *       (src/ORBmatcher.cc:1342-1474; Tracking::TrackWithMotionModel; the 2*th retry stays with the caller);
 *   pgorb_search_by_projection_keyframe_pose   all of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
 *       (src/ORBmatcher.cc:1476-1603; Tracking::Relocalization).
 * Common inputs.  The frame as above: keypoints (mvKeysUn), descriptors, n and the Frame's float bounds.  pose: the frame's pose
 * and camera as ONE pgorb_kf_pose (declared with pgorb_create_new_map_points below): Tcw = rows 0-2 of mTcw, Ow = mOw =
 * -Rcw.t()*tcw formed by the caller exactly as for pgorb_fuse, fx, fy, cx, cy; invfx / invfy are not read.  The table: points
 * (pgorb_map_point: the plain mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance), point_desc [npoints][32], point_bad
 * [npoints] (NULL = none bad) and point_has_obs [npoints] (Observations() > 0; NULL = all 1); no observation lists.  Queries are
 * table indices.  assigned[i] = the index of the QUERY written to mvpMapPoints[i] by this call, or -1; the return value is
 * nmatches.
 *   (a) pgorb_search_local_points.  kp_point[i] = the table index of mCurrentFrame.mvpMapPoints[i] on entry or -1 (NULL = all
 *       -1); queries[q] = mvpLocalMapPoints as table indices, distinct; query_seen[q] (NULL = none) is set for a point whose
 *       mnLastFrameSeen already equals this frame's id for a reason the slots do not show (the outliers discarded at
 *       Tracking.cc:781 and :904); viewing_cos_limit 0.5f, th 1, 3 or 5, nnratio 0.8f.  First loop (:1137-1153): a slot holding a
 *       bad point is cleared, any other slot marks its point as seen.  Second loop (:1158-1171): a seen or bad query is skipped,
 *       every other query runs isInFrustum.  in_view[q] = mbTrackInView (IncreaseVisible from it and from the slots is
 *       pgorb_increase_visible_batch_device); proj_x, proj_y, level, view_cos [nq] (each may be NULL) = mTrackProjX / Y, mnTrackScaleLevel, mTrackViewCos of an
 *       in-view query and 0 for any other; kp_point_out [n] (may be NULL) = the slots after the first loop; *n_to_match (may be
 *       NULL) = nToMatch.  The matcher then runs with those values, kp_has_point[i] = the slot's point after clearing has
 *       point_has_obs set.  (The reference skips the matcher when nToMatch == 0; the result, all -1 and 0, is the same.)
 *   (b) pgorb_search_by_projection_last_frame.  Query i is the last frame's keypoint i (assigned holds last-frame keypoint
 *       indices): last_kps[i].octave is read as mvKeys[i].octave and .angle as mvKeysUn[i].angle; last_point[i] = table index or
 *       -1; last_outlier [nlast] (NULL = none); kp_has_point [n] as in pgorb_search_by_projection_frame (NULL after
 *       TrackWithMotionModel's fill(NULL)).  As in the reference there is NO isBad() test (a bad point is projected and matched),
 *       invzc = (float)(1.0 / z) and invzc < 0 skips, the bounds test is inclusive on both sides, and for mono neither bForward
 *       nor bBackward holds, so tlc is not formed.  valid, u, v [nlast] (each may be NULL): valid[i] = the point went on to the
 *       window search; (u, v) its projection, 0 when not valid.
 *   (c) pgorb_search_by_projection_keyframe_pose.  kf_kps[i].angle is pKF->mvKeysUn[i].angle; kf_point[i] = the table index of
 *       GetMapPointMatches()[i] or -1; already_found [nkf] (NULL = none); kp_has_point as in pgorb_search_by_projection_keyframe
 *       (any point blocks a keypoint).  Bad and found points are skipped; there is NO depth-sign test (a point behind the camera
 *       whose projection lands inside the bounds goes on, as in the reference); dist3D = cv::norm(x3Dw - Ow); the depth test and
 *       PredictScale are those of pgorb_search_by_projection_keyframe.  u, v, dist3d [nkf] (each may be NULL): the projection
 *       and distance of every point that is not NULL, bad or found and projects inside the bounds, 0 for any other.
 * Float readings: DESIGN.md section 4 (the Fuse rows and the tracking rows).  A NaN projection (z = +-0 with a zero numerator, or
 * inf - inf) makes the reference convert NaN to int inside GetFeaturesInArea, which is undefined; pgorb skips such a point (not in
 * view / not valid).  An infinite u fails the bounds test as written.
 * PGORB_E_ARG (single calls, checked on the host before anything else): a negative count, a NULL array that is read, empty bounds,
 * th <= 0, a table index outside [-1, npoints) -- for the queries of (a) outside [0, npoints) -- and in (a) a repeated query.  The
 * batched forms do not check: an index outside [0, npoints) counts as NULL.
 * Limits (PGORB_E_LIMIT): those of the deciding kernel above, keypoints * 13 + queries * 10 + 256 <= 163840 bytes and 16000 for
 * each count (queries = nq, nlast, nkf; in the batched forms of (b) and (c) a pair's queries are a frame of the batch, so
 * cap_per_frame * 23 + 256 <= 163840: 7112); and in (a) npoints <= 1048576: the seen marks are one bit per table point and pair
 * (npairs * 128 KiB of the context's scratch arena at that size). */
struct pgorb_kf_pose;
struct pgorb_map_point;
int  pgorb_search_local_points(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x, float min_y, float max_y,
        const struct pgorb_kf_pose* pose, const int32_t* kp_point /*[n] or NULL*/,
        int npoints, const struct pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad,
        const uint8_t* point_has_obs, int nq, const int32_t* queries, const uint8_t* query_seen,
        float viewing_cos_limit, float th, float nnratio,
        uint8_t* in_view /*[nq]*/, float* proj_x, float* proj_y, int32_t* level, float* view_cos,
        int32_t* kp_point_out /*[n] or NULL*/, int32_t* n_to_match, int32_t* assigned /*[n]*/);
int  pgorb_search_by_projection_last_frame(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x, float min_y, float max_y,
        const struct pgorb_kf_pose* pose, const uint8_t* kp_has_point,
        const pgorb_keypoint* last_kps, int nlast, const int32_t* last_point, const uint8_t* last_outlier,
        int npoints, const struct pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_has_obs,
        float th, int check_orientation, uint8_t* valid, float* u, float* v, int32_t* assigned /*[n]*/);
int  pgorb_search_by_projection_keyframe_pose(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, float min_x, float max_x, float min_y, float max_y,
        const struct pgorb_kf_pose* pose, const uint8_t* kp_has_point,
        const pgorb_keypoint* kf_kps, int nkf, const int32_t* kf_point, const uint8_t* already_found,
        int npoints, const struct pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad,
        float th, int orb_dist, int check_orientation, float* u, float* v, float* dist3d, int32_t* assigned /*[n]*/);
/* Batched, resident forms (the single calls are one-pair batches of these).  Frames and grids as for the batched matchers above;
 * pair p matches into frame d_pair_frame[p] (NULL: frame p) under d_pose[p]; the table is shared by all pairs.  (a): d_kp_point,
 * d_kp_point_out [npairs][cap_per_frame]; d_queries, d_query_seen and the per-query outputs [npairs][qcap] with d_nq[p] entries in
 * use (entries past d_nq[p] are not written); d_n_to_match [npairs]; d_in_view and d_n_to_match are required here.  (b), (c): the last frame / key frame of pair p is frame
 * d_pair_last[p] / d_pair_kf[p] of the same batch; d_last_point, d_last_outlier, d_kf_point, d_already_found and the per-query
 * outputs are [npairs][cap_per_frame], d_kp_has_point [npairs][cap_per_frame] (NULL = none).  d_assigned [npairs][cap_per_frame],
 * d_nmatches [npairs].  One lane per (pair, query) projects (k_track_front) and writes the query arrays the two passes of
 * SearchByProjection read, in the context's scratch arena. */
int  pgorb_search_local_points_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, int npairs,
        float min_x, float max_x, float min_y, float max_y, const struct pgorb_kf_pose* d_pose, const int32_t* d_kp_point,
        int npoints, const struct pgorb_map_point* d_points, const uint8_t* d_point_desc, const uint8_t* d_point_bad,
        const uint8_t* d_point_has_obs, int qcap, const int32_t* d_nq, const int32_t* d_queries, const uint8_t* d_query_seen,
        float viewing_cos_limit, float th, float nnratio,
        uint8_t* d_in_view, float* d_proj_x, float* d_proj_y, int32_t* d_level, float* d_view_cos,
        int32_t* d_kp_point_out, int32_t* d_n_to_match, int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);
int  pgorb_search_by_projection_last_frame_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, const int32_t* d_pair_last, int npairs,
        float min_x, float max_x, float min_y, float max_y, const struct pgorb_kf_pose* d_pose, const uint8_t* d_kp_has_point,
        const int32_t* d_last_point, const uint8_t* d_last_outlier,
        int npoints, const struct pgorb_map_point* d_points, const uint8_t* d_point_desc, const uint8_t* d_point_has_obs,
        float th, int check_orientation, uint8_t* d_valid, float* d_u, float* d_v,
        int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);
int  pgorb_search_by_projection_keyframe_pose_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_frame, const int32_t* d_pair_kf, int npairs,
        float min_x, float max_x, float min_y, float max_y, const struct pgorb_kf_pose* d_pose, const uint8_t* d_kp_has_point,
        const int32_t* d_kf_point, const uint8_t* d_already_found,
        int npoints, const struct pgorb_map_point* d_points, const uint8_t* d_point_desc, const uint8_t* d_point_bad,
        float th, int orb_dist, int check_orientation, float* d_u, float* d_v, float* d_dist3d,
        int32_t* d_assigned, int32_t* d_nmatches, void* hip_stream);

/* ---- Motion-only pose refinement of the tracking thread (csrc/pose_opt.hip) ---------------------------------------------------
 *   pgorb_pose_optimization   Optimizer::PoseOptimization(pFrame) (src/Optimizer.cc:239-451) with the g2o path under it (the vertex
 *       SE3Quat, EdgeSE3ProjectXYZOnlyPose, RobustKernelHuber, OptimizationAlgorithmLevenberg, LinearSolverDense), monocular
 *       (mvuRight < 0), in double.  It is this project's READING of g2o and Eigen (DESIGN.md section 4 lists it), anchored by the
 *       CPU tests of tests/test_pose_optimization.py and not pinned to a g2o build.
 * Inputs.  kps = mvKeysUn (pt and octave are read), pose = the frame's pose and camera as for the matchers above (Tcw, fx, fy, cx,
 * cy are read; invfx / invfy / Ow are not), kp_point[i] = the table index of mvpMapPoints[i] or -1, the table as above (pos is
 * read), point_has_obs [npoints] (NULL = all 1).  invSigma2 is the context's float mvInvLevelSigma2[octave].
 * Outputs.  pose_out = the input with Tcw and Ow = -Rcw.t()*tcw replaced (a complete pgorb_kf_pose for the next call);
 * outlier[i] = mvbOutlier[i] (0 where there is no point); chi2[i] (may be NULL) = the float chi2 of the last classification, 0
 * where there is no point; info (may be NULL) = PGORB_PO_INFO int32: status bits, rounds run, iterations of rounds 0..3, Levenberg
 * trials, edges.  The return value is nInitialCorrespondences - nBad of the last round run.
 *   discard_outliers = 1: the loop after the call in TrackReferenceKeyFrame / TrackWithMotionModel (Tracking.cc:768-787, :891-911)
 *       runs too: kp_point_out[i] = -1 for an outlier slot and its flag is cleared.
 *   discard_outliers = 0: kp_point_out = kp_point (TrackLocalMap, :932-950).
 *   *nmatches_map (may be NULL) = the slots that are not outliers and whose point has point_has_obs, in both forms.
 * PGORB_PO_FEW: fewer than 3 correspondences -- returns 0, pose_out = pose byte for byte, the flags are cleared.
 * PGORB_PO_NONFINITE: the active chi2 a Levenberg iteration starts from, or an edge's chi2 at a classification, is not finite (a
 * point at z = 0; the reference's behaviour there is undefined) -- pose_out = pose byte for byte, every flag and chi2 0, returns 0.
 * Determinism: a problem's result depends on its inputs only, not on its place in a batch, the number of problems, the stream or a
 * repeat; the single call equals the batched one byte for byte (DESIGN.md section 4 states the summation order).
 * PGORB_E_ARG (single call, checked on the host before anything else): a negative count, a NULL array that is read, a slot index
 * outside [-1, npoints), the octave of a slot that holds a point outside the context's levels, a value of Tcw, fx, fy, cx, cy or of
 * a referenced point that is not finite, fx or fy zero.  The batched form does not check: a bad index or octave counts as no point.
 * PGORB_E_LIMIT: more than 16000 keypoints per frame (cap_per_frame in the batched form).
 *   pgorb_slots_from_assignment   kp_point[i] = source[assigned[i]] where assigned[i] >= 0 and untouched elsewhere: the matchers'
 *       `assigned` (indices of queries) back to table indices; source = last_point after the last-frame search, queries after
 *       pgorb_search_local_points.  PGORB_E_ARG: an assignment outside [-1, nsource).  The batched form reads source
 *       [npairs][source_stride] and skips an assignment outside [0, source_stride). */
#define PGORB_PO_FEW        1
#define PGORB_PO_NONFINITE  2
#define PGORB_PO_INFO       8
int  pgorb_pose_optimization(pgorb_ctx* ctx, const pgorb_keypoint* kps, int n,
        const struct pgorb_kf_pose* pose, const int32_t* kp_point /*[n]*/,
        int npoints, const struct pgorb_map_point* points, const uint8_t* point_has_obs, int discard_outliers,
        struct pgorb_kf_pose* pose_out, uint8_t* outlier /*[n]*/, int32_t* kp_point_out /*[n] or NULL*/,
        int32_t* nmatches_map, float* chi2 /*[n] or NULL*/, int32_t* info);
/* pair p refines frame d_pair_frame[p] (NULL: frame p) from d_pose[p]; d_kp_point, d_outlier, d_kp_point_out, d_chi2
 * [npairs][cap_per_frame] (every entry is written), d_pose_out, d_nmatches_map, d_ninliers [npairs], d_info [npairs][PGORB_PO_INFO].
 * One workgroup per pair; the edge records live in the context's scratch arena (32 bytes per pair and keypoint). */
int  pgorb_pose_optimization_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_pair_frame, int npairs, const struct pgorb_kf_pose* d_pose, const int32_t* d_kp_point,
        int npoints, const struct pgorb_map_point* d_points, const uint8_t* d_point_has_obs, int discard_outliers,
        struct pgorb_kf_pose* d_pose_out, uint8_t* d_outlier, int32_t* d_kp_point_out, int32_t* d_nmatches_map, float* d_chi2,
        int32_t* d_info, int32_t* d_ninliers, void* hip_stream);
int  pgorb_slots_from_assignment(pgorb_ctx* ctx, const int32_t* assigned, const int32_t* source, int nsource,
        int32_t* kp_point /*[n] in/out*/, int n);
int  pgorb_slots_from_assignment_batch_device(pgorb_ctx* ctx, const int32_t* d_assigned, const int32_t* d_source, int source_stride,
        int32_t* d_kp_point /*in/out*/, int cap_per_frame, int npairs, void* hip_stream);

/* ---- Matcher of the local-mapping thread ------------------------------------------------------------------------------
 *   pgorb_search_for_triangulation   ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo = false)
 *       src/ORBmatcher.cc:659-825 with CheckDistEpipolarLine :142-159, monocular (mvuRight < 0) -- called by
 *       LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:266) for every covisible neighbour of a new key frame.  Keypoints
 *       are the undistorted mvKeysUn of each key frame, FeatureVectors the CSR arrays pgorb_bow_vectors /
 *       pgorb_feature_vectors_batch_device produce.  F12 = F12.at<float>(r, c) row-major and the epipole (ex, ey) in KF2 are what
 *       the caller's pose arithmetic produced (:665-672, LocalMapping::ComputeF12 :538-555, cv::Mat float).  has_point1[i] /
 *       has_point2[j] = GetMapPoint(i) != NULL, bad or not (:701-705, :724-728); NULL = no keypoint has one.  The thresholds
 *       come from the context: 100*mvScaleFactors[octave] (float) and 3.84*mvLevelSigma2[octave] (double); octaves are taken
 *       to lie in [0, levels).  matches12[i] = the KF2 keypoint matched to KF1 keypoint i, or -1; the reference's vMatchedPairs
 *       are the (i, matches12[i] >= 0) in ascending i.  Returns nmatches.
 *       Exact: every float operation in the reference's order, the epipolar comparison in double, fp32 denormals kept.  Like the
 *       reference, a KF2 keypoint may be matched to several KF1 keypoints (vbMatched2 is never set, :679, :727), and among the
 *       candidates that pass the last one of the smallest distance wins (bestDist only moves on a passing candidate, :753-757).
 *       Each pair equals the reference called with those masks: CreateNewMapPoints adds map points to KF1 between neighbours
 *       (LocalMapping.cc:441), so reproducing that loop exactly means one call per neighbour with the updated has_point1, or
 *       pgorb_create_new_map_points for the whole loop. */
int  pgorb_search_for_triangulation(pgorb_ctx* ctx,
        const pgorb_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_point1, int n1,
        const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1,
        const pgorb_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_point2, int n2,
        const uint32_t* fv2_node, const int32_t* fv2_start, const uint32_t* fv2_feat, int nfv2,
        const float F12[9], float ex, float ey, int check_orientation, int32_t* matches12 /*[n1]*/);
/* Batched, resident: pair p matches key frame d_pair_kf1[p] against d_pair_kf2[p] of one batch in the layout of
 * pgorb_extract_batch_device, FeatureVectors as pgorb_feature_vectors_batch_device writes them.  d_F12 [npairs][9],
 * d_epipole [npairs][2]; d_has_point1 / d_has_point2 [npairs][cap_per_frame] (NULL = none); d_matches12
 * [npairs][cap_per_frame], d_nmatches [npairs].  One wave per (pair, common vocabulary node), then one finishing wave per pair
 * (KF1's mask, the count, the rotation histogram).  Like pgorb_search_by_bow_batch_device, this form does not check the
 * FeatureVectors: keypoints, descriptors and masks are reached only through them, so d_nfv / d_fv_* must be what
 * pgorb_feature_vectors_batch_device writes (every feature index below the frame's d_n, at most cap_per_frame); the single call
 * checks its host FeatureVectors instead (PGORB_E_ARG). */
int  pgorb_search_for_triangulation_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
        const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs, const float* d_F12, const float* d_epipole,
        const uint8_t* d_has_point1, const uint8_t* d_has_point2, int check_orientation,
        int32_t* d_matches12, int32_t* d_nmatches, void* hip_stream);

/* ---- Triangulation of the local-mapping thread -----------------------------------------------------------------------
 *   pgorb_create_new_map_points   LocalMapping::CreateNewMapPoints() (src/LocalMapping.cc:209-454), monocular (mbMonocular,
 *       mvuRight < 0): for every neighbour in the given order the baseline test (:243-262, baseline / medianDepthKF2 < 0.01),
 *       ComputeF12 (:538-555) and the epipole (ORBmatcher.cc:665-672), SearchForTriangulation with ORBmatcher(0.6, false)
 *       (:217, :266; rotation histogram off), then per match the parallax test, the linear triangulation (cv::SVD of a 4x4,
 *       :311-327), the depth, reprojection and scale-consistency tests (:342-423) and, for a point that passes, what
 *       MapPoint::UpdateNormalAndDepth (MapPoint.cc:347-387) stores.  The stereo branches and UnprojectStereo are out of scope.
 *       The precision of every cv::Mat step is a recalled reading of OpenCV 2.4.9, listed in DESIGN.md section 4.
 *   Inputs per key frame: keypoints (mvKeysUn), descriptors, FeatureVector CSR, has_point[i] = GetMapPoint(i) != NULL (NULL =
 *   none), the pose and camera (pgorb_kf_pose), and per neighbour medianDepthKF2 = ComputeSceneMedianDepth(2) (it reads KF2's
 *   map points: pgorb_scene_median_depth_batch_device writes it from the slots and the table).  Neighbours are distinct key frames other than KF1 (GetBestCovisibilityKeyFrames).
 *   Equivalence with the reference's loop: the matcher has vbMatched2 never set (ORBmatcher.cc:679, 727) and no rotation
 *   histogram, so KF1's mask only decides whether keypoint idx1 is searched, not which KF2 keypoint it takes; a pair's
 *   triangulation depends only on the two key frames; a new point changes only KF1 and the current KF2.  So KF1 keypoint idx1
 *   gets the point of the FIRST neighbour (in the given order) whose match for idx1 triangulates, provided idx1 had no point on
 *   entry: every pair is matched and triangulated at once, then the first success per idx1 is kept.
 *   Outputs: points[] in the reference's creation order (neighbour order, then ascending idx1), at most one per idx1, so at
 *   most n1; count[s] = the points made with neighbour s, or PGORB_CNM_SKIPPED when the baseline test skipped it; F12 / epipole
 *   (may be NULL) = ComputeF12 and the epipole of every neighbour, skipped or not; has_point1_out = KF1's mask afterwards.
 *   Two KF1 keypoints may match one KF2 keypoint: both points are listed and KF2's slot ends with the later one (AddMapPoint
 *   overwrites).  Left to the caller: AddObservation / AddMapPoint / Map::AddMapPoint / mlpRecentAddedMapPoints;
 *   ComputeDistinctiveDescriptors (with two observations the reference picks by KeyFrame* address) is one
 *   pgorb_refresh_map_points call over the new points, with the lists in that order.  CheckNewKeyFrames()'s
 *   early return between neighbours (:240) is the caller's choice of how many neighbours to pass.
 *   Returns the number of points, or a PGORB_E_* code.  At most PGORB_CNM_MAX_NEIGHBOURS neighbours, 16000 keypoints. */
#define PGORB_CNM_MAX_NEIGHBOURS 64
#define PGORB_CNM_SKIPPED (-1)
typedef struct pgorb_kf_pose {
    float Tcw[12];           /* [R | t] row-major, GetPose() rows 0-2 */
    float Ow[3];             /* GetCameraCenter() */
    float fx, fy, cx, cy, invfx, invfy;
} pgorb_kf_pose;
typedef struct pgorb_new_map_point {
    int32_t neighbour;       /* slot of the neighbour (pKF2) in the given order */
    int32_t idx1, idx2;      /* keypoint of KF1 and of the neighbour */
    float pos[3];            /* mWorldPos = x3D */
    float normal[3];         /* mNormalVector */
    float min_distance, max_distance;   /* mfMinDistance, mfMaxDistance */
} pgorb_new_map_point;
int  pgorb_create_new_map_points(pgorb_ctx* ctx,
        const pgorb_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_point1, int n1,
        const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1, const pgorb_kf_pose* pose1,
        int nneigh, const pgorb_keypoint* const* kps2, const uint8_t* const* desc2, const uint8_t* const* has_point2,
        const int32_t* n2, const uint32_t* const* fv2_node, const int32_t* const* fv2_start, const uint32_t* const* fv2_feat,
        const int32_t* nfv2, const pgorb_kf_pose* pose2 /*[nneigh]*/, const float* median_depth2 /*[nneigh]*/,
        pgorb_new_map_point* points /*[n1]*/, int32_t* count /*[nneigh]*/, float* F12 /*[nneigh][9] or NULL*/,
        float* epipole /*[nneigh][2] or NULL*/, uint8_t* has_point1_out /*[n1] or NULL*/);
/* Batched, resident: problem k has current key frame d_kf1[k] and neighbours d_neigh[k][0 .. d_nneigh[k]) (frame indices of
 * one batch in the layout of pgorb_extract_batch_device, FeatureVectors as pgorb_feature_vectors_batch_device writes them,
 * unchecked as in pgorb_search_for_triangulation_batch_device).  d_pose [nframes], d_has_point [nframes][cap_per_frame] (NULL
 * = none), d_median_depth [nkf][max_neigh].  Outputs: d_points [nkf][cap_per_frame], d_npoints [nkf], d_count
 * [nkf][max_neigh] (0 past d_nneigh[k]), d_F12 [nkf][max_neigh][9] and d_epipole [nkf][max_neigh][2] (may be NULL),
 * d_has_point1_out [nkf][cap_per_frame] (may be NULL).  Each problem equals the reference called with the masks it was
 * given: the reference runs key frames one after another and each changes its neighbours' masks, so problems whose key frames
 * neighbour each other are the caller's to order. */
int  pgorb_create_new_map_points_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
        const pgorb_kf_pose* d_pose, const uint8_t* d_has_point, const int32_t* d_kf1, int nkf, const int32_t* d_neigh,
        const int32_t* d_nneigh, int max_neigh, const float* d_median_depth,
        pgorb_new_map_point* d_points, int32_t* d_npoints, int32_t* d_count, float* d_F12, float* d_epipole,
        uint8_t* d_has_point1_out, void* hip_stream);

/* ---- Fusion of duplicate map points of the local-mapping thread -------------------------------------------------------
 *   pgorb_fuse   ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th) (src/ORBmatcher.cc:827-979),
 *       monocular (mvuRight < 0), with KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:672-716) and what Fuse reads
 *       and changes of a MapPoint: Observations() (MapPoint.cc:119-130), Replace (:196-232), IsInKeyFrame and the distance
 *       getters (:402-417 and :390-400).  Call sites: LocalMapping::SearchInNeighbors fuses the new key frame's points into
 *       every target (src/LocalMapping.cc:491) and the targets' points back into the new key frame (:516).
 *   The map points Fuse reads live in one TABLE shared by the queries and the key frame's slots: per point its pose fields
 *   (pgorb_map_point: the plain mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance, not the *Invariance() getters), its
 *   32-byte descriptor, a bad flag and its observations as CSR: obs_kf[obs_start[i] .. obs_start[i + 1]) = the KeyFrame::mnId
 *   of every key frame observing point i, ascending and without repeats (monocular: Observations() is their number).  The key
 *   frame is its undistorted keypoints (mvKeysUn), descriptors, pose and camera, its mnId kf_id, and its slots:
 *   kf_point[i] = the table index of GetMapPoint(i), or -1.  queries[q] = the table index of vpMapPoints[q], or -1 for NULL.
 *   The bounds are the Frame's (the grid is built from them, Frame.cc:216-217); the key frame keeps them as int
 *   (KeyFrame.h:195-198), and IsInImage (x >= minX && x < maxX, strict on the max side) and the search window read those.
 *   Exact decomposition.  Given distinct non-NULL queries and consistent slots (a live point in slot i
 *   lists kf_id, and no live point holds two slots): (1) what a query matches depends only on its own state and the key frame's,
 *   and an earlier query changes another point's state only as the loser or survivor of a Replace -- the loser is the query or
 *   the slot's occupant, the survivor's new descriptor is read by no later query (occupants are in pKF and so skipped) -- so
 *   every query's (bestIdx, bestDist) comes from the state on entry, all at once; (2) a query with bestDist <= TH_LOW (50)
 *   touches only slot bestIdx, so each slot's chain of queries is walked on its own, in query order.  Per query, action[q]:
 *     PGORB_FUSE_SKIPPED            NULL, bad, already in pKF, or a test before the descriptor loop failed (no candidate);
 *     PGORB_FUSE_NO_MATCH           candidates, but no distance <= 50 among those that pass the octave and chi-square tests;
 *     PGORB_FUSE_ADDED              empty slot: pMP->AddObservation(pKF, bestIdx); pKF->AddMapPoint(pMP, bestIdx);
 *     PGORB_FUSE_MERGED_INTO_KF_POINT   occupant.Observations() > query's: pMP->Replace(pMPinKF), the query becomes bad;
 *     PGORB_FUSE_REPLACED_KF_POINT      otherwise (ties included): pMPinKF->Replace(pMP), the query takes the slot;
 *     PGORB_FUSE_KF_POINT_BAD       the occupant is bad: nothing changes, but the query counts toward nFused.
 *   After a Replace the survivor observes the UNION of both key-frame sets; a chain's counts follow those sets.
 *   best_idx / best_dist (may be NULL) = -1 / -1 for a skipped query, -1 / 256 when no candidate passed; kf_point_out (may be
 *   NULL) = the slots afterwards.  Returns nFused or a PGORB_E_* code.  The caller replays the actions in query order against
 *   its own map: Replace, AddObservation / AddMapPoint, IncreaseFound / IncreaseVisible, Map::EraseMapPoint; the survivors'
 *   ComputeDistinctiveDescriptors is pgorb_refresh_map_points (below).  PGORB_E_ARG: an index out of range, an observation list unsorted or
 *   with repeats, a repeated non-NULL query, a live (not bad) occupant that does not list kf_id or holds two slots, th <= 0.  The search
 *   level comes from MapPoint::PredictScale under pgorb_log_f with the context's mfLogScaleFactor; octaves lie in [0, levels). */
#define PGORB_FUSE_SKIPPED 0
#define PGORB_FUSE_NO_MATCH 1
#define PGORB_FUSE_ADDED 2
#define PGORB_FUSE_MERGED_INTO_KF_POINT 3
#define PGORB_FUSE_REPLACED_KF_POINT 4
#define PGORB_FUSE_KF_POINT_BAD 5
typedef struct pgorb_map_point {
    float pos[3];            /* mWorldPos */
    float normal[3];         /* mNormalVector */
    float min_distance, max_distance;   /* mfMinDistance, mfMaxDistance */
} pgorb_map_point;
int  pgorb_fuse(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* pose, uint64_t kf_id,
        float min_x, float max_x, float min_y, float max_y, const int32_t* kf_point /*[n] or NULL = all empty*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_desc /*[npoints][32]*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        const int32_t* obs_start /*[npoints + 1]*/, const uint64_t* obs_kf, int nq, const int32_t* queries /*[nq]*/, float th,
        int32_t* action /*[nq]*/, int32_t* best_idx /*[nq] or NULL*/, int32_t* best_dist /*[nq] or NULL*/,
        int32_t* kf_point_out /*[n] or NULL*/);
/* Batched, resident: problem p fuses its queries d_queries[p][0 .. d_nq[p]) into key frame d_kf[p] of one batch in the layout of
 * pgorb_extract_batch_device, grids as pgorb_frame_grid_batch_device writes them (with the same bounds).  d_kf_id and d_pose
 * are [nframes], d_kf_point [nframes][cap_per_frame] (NULL = every slot empty); the map-point table as above, on the device.
 * Outputs: d_action, d_best_idx, d_best_dist [nprob][qcap] (the last two may be NULL; entries past d_nq[p] are not written),
 * d_kf_point_out [nprob][cap_per_frame] (may be NULL), d_nfused [nprob].  This form does not check its inputs: indices out of
 * range count as NULL / empty, but the observation lists must be what the single call accepts.  Each problem equals the
 * reference called on the state it was given: the reference runs the targets of SearchInNeighbors one after another and each
 * changes bad flags, observation sets and (through ComputeDistinctiveDescriptors) descriptors of the points it fuses, so
 * problems that share a key frame or a map point are the caller's to order.  One lane per query matches (k_fuse_match), then
 * one workgroup per problem walks the slots' chains (k_fuse_resolve). */
int  pgorb_fuse_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf /*[nprob]*/, int nprob,
        const uint64_t* d_kf_id, const pgorb_kf_pose* d_pose, float min_x, float max_x, float min_y, float max_y,
        const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
        const uint8_t* d_point_bad, const int32_t* d_obs_start, const uint64_t* d_obs_kf,
        int qcap, const int32_t* d_nq, const int32_t* d_queries, float th,
        int32_t* d_action, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_kf_point_out, int32_t* d_nfused,
        void* hip_stream);

/* ---- Loop closing: the two Scw matchers, then SearchByBoW(KF, KF) and SearchBySim3 -------------------------------------------------------------------------------------
 * Both take the key frame as pgorb_fuse does (undistorted mvKeysUn, descriptors, the Frame's bounds, of which the key frame's
 * int copies serve IsInImage -- strict on the max side -- and KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:672-716), the
 * map-point TABLE of pgorb_fuse without observation lists (pose fields with the plain mfMin/MaxDistance, descriptor, bad flag),
 * and the DECOMPOSED Scw of :301-305 / :990-994 as a pgorb_kf_pose: Tcw = [Rcw | tcw] with Rcw = sRcw/scw and tcw =
 * Scw(0..2, 3)/scw, Ow = -Rcw.t()*tcw, and the key frame's camera.  Those once-per-call cv::Mat steps stay with the owner of
 * the Sim3.  Per query, in this order: bad or in spAlreadyFound; z < 0; IsInImage; the depth range 0.8f*mfMinDistance ..
 * 1.2f*mfMaxDistance on cv::norm(p3Dw - Ow); PO.dot(Pn) < 0.5*dist in double; MapPoint::PredictScale under pgorb_log_f with the
 * context's mfLogScaleFactor; radius th*mvScaleFactors[level]; octaves [level - 1, level], taken to lie in [0, levels); the
 * first smallest descriptor distance (strict <); bestDist <= TH_LOW (50).  No chi-square test.  The float / double readings are
 * Fuse's.  queries[q] = a table index; unlike pgorb_fuse a point MAY be queried twice (the reference
 * does not forbid it).  spAlreadyFound is the state on entry and is never updated (:308, :997).
 *
 *   pgorb_search_by_projection_sim3   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:
 *       292-405; LoopClosing::ComputeSim3, src/LoopClosing.cc:375, th = 10).  matched_in[i] = the table index of vpMatched[i] or
 *       -1 (NULL = all -1); spAlreadyFound = the set of those.  Candidates whose vpMatched[idx] is set are skipped (:377), and an
 *       accepted query sets it: THE ROUTINE DEPENDS ON ORDER, a later query takes its next best.  Outputs: assigned[i] = the
 *       query index whose point this call wrote into vpMatched[i], or -1; matched_out (may be NULL) = vpMatched afterwards.
 *       Returns nmatches.  Exact decomposition: a query takes its smallest-distance untaken candidate only if that distance is
 *       <= 50, so candidates above 50 are dropped from the lists without changing any decision; the lists of all queries are
 *       built in parallel in the reference's scan order, then one workgroup per problem decides the queries in rounds of
 *       provably independent ones (a query is decided once no undecided earlier query lists any of its untaken candidates).
 *   pgorb_fuse_sim3   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:981-1104;
 *       LoopClosing::SearchAndFuse, src/LoopClosing.cc:601, th = 4, once per connected key frame).  kf_point[i] = the table index
 *       of GetMapPoint(i) or -1 (NULL = all empty); spAlreadyFound = GetMapPoints() on entry.  IsInKeyFrame is not consulted and
 *       no Replace happens here, so no observation lists.  action[q]: PGORB_FUSE_SKIPPED (bad, already found, or a test before
 *       the descriptor loop failed), PGORB_FUSE_NO_MATCH, PGORB_FUSE_ADDED (the slot was empty: AddObservation + AddMapPoint),
 *       PGORB_FUSE_KF_POINT_BAD (a bad occupant: nothing happens, but the query counts), and PGORB_FUSE_REPLACE_REQUESTED:
 *       vpReplacePoint[q] = pMPinKF, with replace_point[q] = the occupant's table index (-1 for every other action).  Matching
 *       never reads the slots, so it comes from the entry state, one lane per query; per slot the first matched query in list
 *       order finds it empty and is ADDED (an atomicMin of the query index), every later one sees that query's point as the
 *       occupant -- a repeated query then points at itself.  best_idx / best_dist (may be NULL) = -1 / -1 for a skipped query,
 *       -1 / 256 when no candidate passed the octave test; kf_point_out (may be NULL) = the slots afterwards.  Returns nFused.
 *       The caller replays ADDED and, under the map mutex, Replace of the requested points (LoopClosing.cc:607-615).
 *   Single calls: PGORB_E_ARG on an index out of range (queries may not be NULL points: the reference dereferences them), th <= 0,
 *   empty bounds; PGORB_E_LIMIT above 16000 keypoints.
 *   Batched, resident forms: problem p runs its queries d_queries[p][0 .. d_nq[p]) against key frame d_kf[p] of one batch in the
 *   layout of pgorb_extract_batch_device, grids as pgorb_frame_grid_batch_device writes them (same bounds); d_pose [nframes];
 *   d_kf_point [nframes][cap_per_frame] but d_matched_in [nprob][cap_per_frame] (both may be NULL).  Outputs [nprob][qcap]
 *   (action, replace_point, best_idx, best_dist; entries past d_nq[p] are not written) or [nprob][cap_per_frame] (assigned,
 *   matched_out, kf_point_out), counts [nprob].  These forms do not check their inputs: indices out of range count as NULL /
 *   empty.  Problems that share a key frame see the same entry state; ordering them is the caller's. */
#define PGORB_FUSE_REPLACE_REQUESTED 6
int  pgorb_search_by_projection_sim3(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* scw_pose,
        float min_x, float max_x, float min_y, float max_y, const int32_t* matched_in /*[n] or NULL*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_desc /*[npoints][32]*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        int nq, const int32_t* queries /*[nq]*/, int th, int32_t* assigned /*[n]*/, int32_t* matched_out /*[n] or NULL*/);
int  pgorb_search_by_projection_sim3_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf /*[nprob]*/, int nprob,
        const pgorb_kf_pose* d_scw_pose, float min_x, float max_x, float min_y, float max_y,
        const int32_t* d_matched_in, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
        const uint8_t* d_point_bad, int qcap, const int32_t* d_nq, const int32_t* d_queries, int th,
        int32_t* d_assigned, int32_t* d_matched_out, int32_t* d_nmatches, void* hip_stream);
int  pgorb_fuse_sim3(pgorb_ctx* ctx,
        const pgorb_keypoint* kps, const uint8_t* desc, int n, const pgorb_kf_pose* scw_pose,
        float min_x, float max_x, float min_y, float max_y, const int32_t* kf_point /*[n] or NULL = all empty*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_desc /*[npoints][32]*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        int nq, const int32_t* queries /*[nq]*/, float th, int32_t* action /*[nq]*/, int32_t* replace_point /*[nq]*/,
        int32_t* best_idx /*[nq] or NULL*/, int32_t* best_dist /*[nq] or NULL*/, int32_t* kf_point_out /*[n] or NULL*/);
int  pgorb_fuse_sim3_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_kf /*[nprob]*/, int nprob,
        const pgorb_kf_pose* d_scw_pose, float min_x, float max_x, float min_y, float max_y,
        const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc,
        const uint8_t* d_point_bad, int qcap, const int32_t* d_nq, const int32_t* d_queries, float th,
        int32_t* d_action, int32_t* d_replace_point, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_kf_point_out,
        int32_t* d_nfused, void* hip_stream);

/*   pgorb_search_by_bow_keyframes   ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (src/ORBmatcher.cc:
 *       524-657; LoopClosing::ComputeSim3, src/LoopClosing.cc:265, once per loop candidate).  Both key frames come as descriptors,
 *       the angles of mvKeysUn, and their FeatureVector CSR arrays (pgorb_bow_vectors / pgorb_feature_vectors_batch_device: node
 *       ids ascending); point_valid1[i] / point_valid2[j] = the keypoint has a map point and it is not bad.  matches12[i1] = the
 *       KF2 keypoint whose map point the reference writes to vpMatches12[i1], or -1; returns nmatches.  Unlike pgorb_search_by_bow:
 *       bestDist1 < TH_LOW is STRICT (:600); the ratio test is on floats (:602); KF2's side is masked by validity and by
 *       vbMatched2 (:578-582), which only an accepted match writes (:605); the rotation bin uses mvKeysUn angles of both.
 *       A KF2 feature belongs to one vocabulary node, so nodes are independent and inside a node KF1's features go in
 *       FeatureVector order: one wave per (pair, common node), then one finishing wave per pair (count, rotation histogram).
 *       The single call checks its FeatureVectors (PGORB_E_ARG: starts not rising from 0, a feature index past n, node ids not
 *       ascending).  THE BATCHED FORM TRUSTS ITS FeatureVectors, as pgorb_search_for_triangulation_batch_device does: d_nfv /
 *       d_fv_* must be what pgorb_feature_vectors_batch_device writes.  d_point_valid1 / 2 and d_matches12 are
 *       [npairs][cap_per_frame], d_nmatches [npairs]. */
int  pgorb_search_by_bow_keyframes(pgorb_ctx* ctx,
        const uint8_t* desc1, const float* angle1, const uint8_t* point_valid1, int n1,
        const uint32_t* fv1_node, const int32_t* fv1_start, const uint32_t* fv1_feat, int nfv1,
        const uint8_t* desc2, const float* angle2, const uint8_t* point_valid2, int n2,
        const uint32_t* fv2_node, const int32_t* fv2_start, const uint32_t* fv2_feat, int nfv2,
        float nnratio, int check_orientation, int32_t* matches12 /*[n1]*/);
int  pgorb_search_by_bow_keyframes_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const uint32_t* d_fv_node, const int32_t* d_fv_start, const uint32_t* d_fv_feat, const int32_t* d_nfv,
        const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs, const uint8_t* d_point_valid1, const uint8_t* d_point_valid2,
        float nnratio, int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, void* hip_stream);

/*   pgorb_search_by_sim3   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1106-1330;
 *       LoopClosing::ComputeSim3, src/LoopClosing.cc:323, th = 7.5).  Per key frame: undistorted keypoints, descriptors, the pose
 *       (Tcw = GetRotation() | GetTranslation(); of pose2 only Tcw is read: BOTH projections use pKF1's fx, fy, cx, cy,
 *       :1109-1112) and the slots kf_point[i] = a table index or -1 (NULL = none) into a pgorb_map_point table (the normal is
 *       unused).  pgorb_sim3 holds the transform as the caller's own cv::Mat arithmetic of :1123-1125 produced it: sR12 = s12*R12,
 *       t12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (row-major); those once-per-call products stay with the owner of the
 *       poses.  already1[i] / already2[j] are vbAlreadyMatched1 / 2 of :1133-1146 (NULL = none); the caller owns
 *       GetIndexInKeyFrame.  Per slot and direction: no point, already matched or bad -> nothing; p3Dc = Rw*p + tw, then sR*p3Dc
 *       + t (gemm's small-matrix path, the translation as C); z < 0; IsInImage of the key frame's int bounds; dist3D = cv::norm
 *       of the CAMERA-FRAME vector (double); the depth range 0.8f*mfMinDistance .. 1.2f*mfMaxDistance; PredictScale; radius
 *       th*mvScaleFactors[level]; octaves [level - 1, level]; the first smallest distance; bestDist <= TH_HIGH (100).  No
 *       viewing-angle and no chi-square test.  match12[i1] = the KF2 keypoint of every NEWLY found pair, those with
 *       vnMatch2[vnMatch1[i1]] == i1 (:1314-1327), or -1; returns nFound.  Nothing depends on order: one lane per (pair,
 *       direction, slot), then one agreement pass.  PGORB_E_ARG: a slot index out of range, th <= 0, empty bounds.
 *       Batched: pair p matches key frames d_pair_kf1[p] and d_pair_kf2[p] of one batch (layout and grids as above);
 *       d_pose and d_kf_point go by frame, d_sim3 [npairs], d_already1 / 2 and d_match12 [npairs][cap_per_frame] (entries past
 *       the key frame's d_n are not written), d_nfound [npairs].  Unchecked: indices out of range count as empty. */
typedef struct pgorb_sim3 { float sR12[9], t12[3], sR21[9], t21[3]; } pgorb_sim3;
int  pgorb_search_by_sim3(pgorb_ctx* ctx,
        const pgorb_keypoint* kps1, const uint8_t* desc1, int n1, const pgorb_kf_pose* pose1, const int32_t* kf_point1, const uint8_t* already1,
        const pgorb_keypoint* kps2, const uint8_t* desc2, int n2, const pgorb_kf_pose* pose2, const int32_t* kf_point2, const uint8_t* already2,
        float min_x, float max_x, float min_y, float max_y,
        int npoints, const pgorb_map_point* points, const uint8_t* point_desc, const uint8_t* point_bad /*[npoints] or NULL*/,
        const pgorb_sim3* sim3, float th, int32_t* match12 /*[n1]*/);
int  pgorb_search_by_sim3_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_grid_start, const int32_t* d_grid_idx, const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs,
        const pgorb_kf_pose* d_pose, float min_x, float max_x, float min_y, float max_y,
        const int32_t* d_kf_point, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_desc, const uint8_t* d_point_bad,
        const pgorb_sim3* d_sim3, const uint8_t* d_already1, const uint8_t* d_already2, float th,
        int32_t* d_match12, int32_t* d_nfound, void* hip_stream);

/*   pgorb_sim3_solver   Sim3Solver (src/Sim3Solver.cc:37-423; LoopClosing::ComputeSim3, src/LoopClosing.cc:274-342): the constructor,
 *       SetRansacParameters and ONE call of iterate(niterations) -- or find(), with niterations >= max_iterations -- of a solver whose
 *       mnIterations and mnBestInliers are first_iteration and best_inliers_in.  It is the step between pgorb_search_by_bow_keyframes
 *       and pgorb_search_by_sim3: matches12 [n1] is exactly what the former writes (the KF2 keypoint or -1), found_sim3 and
 *       already1 / already2 are what the latter reads.  Key frames and the table as for pgorb_search_by_sim3: of the poses Tcw, fx, fy,
 *       cx, cy are read (each key frame's OWN camera, :105-109), kf_point the slots; the caller owns GetIndexInKeyFrame and passes -1
 *       where it would be negative.  Sigma2 is the context's mvLevelSigma2[octave].
 *   The constructor (:37-112).  A correspondence is kept where matches12[i1] = i2 >= 0, kf_point1[i1] and kf_point2[i2] hold points and
 *       neither is bad; kept ones are compacted IN i1 ORDER (the draws index this order): X3Dc = Rcw*P + tcw per key frame, its image
 *       under that key frame's K, and the thresholds: mvnMaxError1/2 are vector<size_t> (Sim3Solver.h:78-79), so 9.210*sigma2 is
 *       evaluated in double, TRUNCATED to an integer and compared as float -- 9 for octave 0, not 9.21.
 *   SetRansacParameters (:114-138).  mRansacMaxIts(N) is evaluated on the host with the reference's own expression (the host's log;
 *       pow of the float epsilon promoted to double) and kept as a table by N in the context, re-made when probability, min_inliers
 *       or max_iterations change; pgorb_sim3_max_iterations returns one entry.  No device logarithm decides a ceil.  nIterations is
 *       an int there: a quotient that is NaN or not below 2^31 becomes INT_MIN (x86-64's cvttsd2si) and the cap 1, so with 20
 *       inliers asked of more than about 15500 correspondences the reference runs one iteration, and so does the library.
 *   iterate (:140-207).  draws [max_iterations][3] are raw rand() values in [0, 2^31); iteration t uses draws[t].  The library applies
 *       RandomInt's formula int((double)r/((double)RAND_MAX + 1.0)*size) (DUtils/Random.cpp:47-50) and the swap-with-back selection of
 *       :166-177, so a caller who seeds rand() as the reference does reproduces it.  All iterations of the window [first_iteration,
 *       min(first_iteration + niterations, mRansacMaxIts)) are evaluated at once; with inl[t] the inlier count of iteration t and
 *       b[t] = max(best_inliers_in, inl[first .. t-1]) the call returns the first t with inl[t] > min_inliers && inl[t] >= b[t]
 *       (PGORB_S3_FOUND), and otherwise `best` is the LAST t with inl[t] >= b[t] -- the reference's `>=` at :183.
 *   ComputeSim3 (:226-337) and CheckInliers (:340-364) follow the cv::Mat readings of DESIGN.md section 4.  cv::eigen is READ as a
 *       cyclic Jacobi in double on the float N with the eigenvector's sign as it falls out (the rotation does not depend on it);
 *       OpenCV 2.4.9 cannot be built here, so this is a reading and not a pin.  A hypothesis with a non-finite
 *       quantity (norm(vec) == 0, den == 0, a point at z == 0) gets what the reference's comparisons give: a NaN compares false.
 * Outputs.  The return value is nInliers (0 without PGORB_S3_FOUND).  found = R12, t12, s12 of the returned hypothesis; found_sim3 the
 * same as the pgorb_sim3 record above (s*R, (1.0/s)*R.t(), -sR21*t12, as :323-335 form them); best = mBestRotation / Translation /
 * Scale after the call (zero when no iteration of the call reached the carried best); inlier [n1] = vbInliers; matches12_out [n1] =
 * matches12 where inlier is set, else -1 (LoopClosing.cc:313-318); already1 [n1] / already2 [n2] (may be NULL) = what SearchBySim3
 * derives from that vector (ORBmatcher.cc:1133-1146).  info (may be NULL) = PGORB_S3_INFO int32: status bits, N, mRansacMaxIts,
 * mnIterations after the call, nInliers, mnBestInliers after the call, the iteration of `best` (-1: none), 0.
 * Without PGORB_S3_FOUND: returns 0, inlier all 0, matches12_out all -1, already1 / 2 all 0, found and found_sim3 zeroed; best and
 * info are still written.  PGORB_S3_FEW: N < min_inliers (bNoMore; nothing evaluated).  PGORB_S3_NO_MORE: not found and mnIterations
 * reached mRansacMaxIts.
 * Determinism: a pair's result depends on its inputs only, not on its place in a batch, the number of pairs, the stream or a repeat;
 * every lane of a hypothesis' wave runs Horn in one fixed operation order, counts are sums of ballot popcounts, there are no atomics;
 * the single call equals the batched one byte for byte.
 * PGORB_E_ARG (single call, checked on the host before anything else): a negative count, a NULL array that is read, a slot outside
 * [-1, npoints), matches12 outside [-1, n2), the octave of a used keypoint outside the context's levels, a value of Tcw, fx, fy, cx,
 * cy or of a referenced point that is not finite, min_inliers < 3, probability outside (0, 1), max_iterations < 1, first_iteration
 * < 0, niterations < 1, a draw >= 2^31.  PGORB_E_LIMIT: more than 16000 keypoints in a key frame (cap_per_frame), max_iterations >
 * PGORB_SIM3_MAX_ITERATIONS.  The batched form checks the parameters and the limits only: a bad index or octave counts as no
 * correspondence.
 *   Batched: pair p aligns key frames d_pair_kf1[p] and d_pair_kf2[p] of one batch; d_pose and d_kf_point go by frame; d_matches12,
 *       d_inlier, d_matches12_out, d_already1 / 2 are [npairs][cap_per_frame] (every entry is written), d_draws
 *       [npairs][max_iterations][3], d_found, d_found_sim3, d_best, d_ninliers [npairs], d_info [npairs][PGORB_S3_INFO];
 *       d_first_iteration / d_best_inliers_in [npairs] or NULL = the params' values.  Three launches; the scratch arena holds 64 bytes
 *       per pair and keypoint and per pair and iteration of the window. */
typedef struct pgorb_sim3_params { float probability; int32_t min_inliers, max_iterations, fix_scale,
                                   first_iteration, niterations, best_inliers_in; } pgorb_sim3_params;
typedef struct pgorb_sim3_estimate { float R12[9], t12[3], s12; } pgorb_sim3_estimate;
#define PGORB_S3_FEW      1   /* N < min_inliers: bNoMore, nothing evaluated */
#define PGORB_S3_FOUND    2
#define PGORB_S3_NO_MORE  4   /* mnIterations reached mRansacMaxIts */
#define PGORB_S3_INFO     8   /* status, N, mRansacMaxIts, mnIterations after the call, nInliers, mnBestInliers, iteration of the best, reserved */
#define PGORB_SIM3_MAX_ITERATIONS 1024
int  pgorb_sim3_max_iterations(float probability, int min_inliers, int max_iterations, int N);
int  pgorb_sim3_solver(pgorb_ctx* ctx,
        const pgorb_keypoint* kps1, int n1, const pgorb_kf_pose* pose1, const int32_t* kf_point1,
        const pgorb_keypoint* kps2, int n2, const pgorb_kf_pose* pose2, const int32_t* kf_point2,
        const int32_t* matches12 /*[n1]: KF2 keypoint or -1*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_bad /*[npoints] or NULL*/,
        const pgorb_sim3_params* params, const uint32_t* draws /*[max_iterations][3]*/,
        pgorb_sim3_estimate* found, pgorb_sim3* found_sim3, pgorb_sim3_estimate* best,
        uint8_t* inlier /*[n1]*/, int32_t* matches12_out /*[n1]*/, uint8_t* already1 /*[n1] or NULL*/, uint8_t* already2 /*[n2] or NULL*/,
        int32_t* info);
int  pgorb_sim3_solver_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, const int32_t* d_kf_point,
        const int32_t* d_matches12, int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_bad,
        const pgorb_sim3_params* params /*host, one for all*/,
        const int32_t* d_first_iteration, const int32_t* d_best_inliers_in /*[npairs] or NULL = the params' values*/,
        const uint32_t* d_draws /*[npairs][max_iterations][3]*/, pgorb_sim3_estimate* d_found, pgorb_sim3* d_found_sim3,
        pgorb_sim3_estimate* d_best, uint8_t* d_inlier, int32_t* d_matches12_out, uint8_t* d_already1, uint8_t* d_already2,
        int32_t* d_info, int32_t* d_ninliers, void* hip_stream);

/*   pgorb_optimize_sim3   Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:1046-1241) with the
 *       g2o path under it (VertexSim3Expmap, EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ with their NUMERIC Jacobian, RobustKernelHuber,
 *       OptimizationAlgorithmLevenberg, LinearSolverDense), in double: step 4 of LoopClosing::ComputeSim3, between pgorb_search_by_sim3
 *       and pgorb_search_by_projection_sim3.  It is this project's READING of g2o and Eigen (DESIGN.md section 4 lists it), anchored
 *       by the CPU tests of tests/test_optimize_sim3.py and not pinned to a g2o build.
 * Inputs.  Both key frames and the table as for pgorb_sim3_solver (Tcw and each key frame's own fx, fy, cx, cy are read; pos and
 * point_bad of the table).  matches12 [n1] = the KF2 keypoint or -1: the solver's matches12_out.  new_matches12 [n1] (may be NULL) =
 * what pgorb_search_by_sim3 wrote: where it is >= 0 it replaces the entry, as the reference's in-place vpMatches12[idx1] = ... does.
 * A correspondence is an entry i1 with a match i2, kf_point1[i1] >= 0, kf_point2[i2] >= 0 and neither point bad; it carries the edge
 * pair e12 (obs1 - cam1(S12 * P2c)) and e21 (obs2 - cam2(S12^-1 * P1c)) with invSigma2 of each keypoint's octave.  estimate = the
 * float R, t, s of LoopClosing.cc:320-325 (the solver's `found`); th2: the reference passes 10; fix_scale = mbFixScale.
 * Outputs.  The return value is nIn.  estimate_out = R12, t12, s12 of the recovered g2o::Sim3 rounded to float.  matches12_out [n1] =
 * the merged input with every removed correspondence set to -1.  chi2_12 / chi2_21 [n1] (may be NULL) = the float chi2 each edge held
 * at its last classification, 0 where there is no edge.  scw_pose (may be NULL) = a complete pgorb_kf_pose for
 * pgorb_search_by_projection_sim3: gScm * gSmw in double with gSmw from pose2 (LoopClosing.cc:333-335), Converter::toCvMat, then the
 * decomposition described there; it carries KF1's camera.  info (may be NULL) = PGORB_OS3_INFO int32: status bits,
 * nCorrespondences, nBad, iterations and Levenberg trials of the first optimize call, the same of the second, nMoreIterations.
 * PGORB_OS3_FEW: nCorrespondences - nBad < 10 -- returns 0 before the vertex is recovered: estimate_out = estimate byte for byte,
 * matches12_out keeps the -1s of the first classification, scw_pose is zeroed.
 * PGORB_OS3_NONFINITE: the active chi2 a Levenberg iteration starts from, or an edge's chi2 at a classification, is not finite --
 * returns 0, estimate_out = estimate byte for byte, matches12_out = the merged input, every chi2 0, scw_pose zeroed.
 * Determinism: a pair's result depends on its inputs only; the single call equals the batched one byte for byte.
 * PGORB_E_ARG (single call, on the host before anything else): a negative count, a NULL array that is read, a slot index outside
 * [-1, npoints), matches12 or new_matches12 outside [-1, n2), the octave of a used keypoint outside the context's levels, a value
 * of Tcw, fx, fy, cx, cy, the estimate or a referenced point that is not finite, th2 <= 0, s12 <= 0.  PGORB_E_LIMIT: more than 16000
 * keypoints in a key frame (cap_per_frame).  The batched form checks th2 and the limits only: a bad index or octave counts as no
 * correspondence.
 *   Batched: pair p refines key frames d_pair_kf1[p] and d_pair_kf2[p]; d_pose and d_kf_point go by frame; d_matches12,
 *       d_new_matches12 (or NULL), d_matches12_out, d_chi2_12 / 21 are [npairs][cap_per_frame] (every entry is written), d_estimate,
 *       d_estimate_out, d_scw_pose, d_nin [npairs], d_info [npairs][PGORB_OS3_INFO].  One launch, one workgroup per pair; the scratch
 *       arena holds 64 bytes per pair and keypoint. */
#define PGORB_OS3_FEW        1
#define PGORB_OS3_NONFINITE  2
#define PGORB_OS3_INFO       8
int  pgorb_optimize_sim3(pgorb_ctx* ctx,
        const pgorb_keypoint* kps1, int n1, const pgorb_kf_pose* pose1, const int32_t* kf_point1,
        const pgorb_keypoint* kps2, int n2, const pgorb_kf_pose* pose2, const int32_t* kf_point2,
        const int32_t* matches12 /*[n1]*/, const int32_t* new_matches12 /*[n1] or NULL*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_bad /*[npoints] or NULL*/,
        const pgorb_sim3_estimate* estimate, float th2, int fix_scale,
        pgorb_sim3_estimate* estimate_out, int32_t* matches12_out /*[n1]*/, float* chi2_12, float* chi2_21 /*[n1] or NULL*/,
        pgorb_kf_pose* scw_pose, int32_t* info);
int  pgorb_optimize_sim3_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_pair_kf1, const int32_t* d_pair_kf2, int npairs, const pgorb_kf_pose* d_pose, const int32_t* d_kf_point,
        const int32_t* d_matches12, const int32_t* d_new_matches12, int npoints, const pgorb_map_point* d_points,
        const uint8_t* d_point_bad, const pgorb_sim3_estimate* d_estimate, float th2, int fix_scale,
        pgorb_sim3_estimate* d_estimate_out, int32_t* d_matches12_out, float* d_chi2_12, float* d_chi2_21,
        pgorb_kf_pose* d_scw_pose, int32_t* d_info, int32_t* d_nin, void* hip_stream);

/*   pgorb_pnp_solver   PnPsolver (src/PnPsolver.cc:67-950, include/PnPsolver.h; Tracking::Relocalization, src/Tracking.cc:1341-1420): the
 *       constructor, SetRansacParameters, one iterate(niterations) (find = iterate(mRansacMaxIts)), Refine, CheckInliers and the EPnP
 *       under compute_pose, monocular.  Step 4 of relocalisation, between pgorb_search_by_bow and pgorb_pose_optimization: kp_point is
 *       what pgorb_slots_from_assignment made of the former's assignment, pose_out / kp_point_out are what the latter reads as pose /
 *       kp_point (Tracking.cc:1405-1420: the PnP pose, and no point where vbInliers is false).  It is this project's READING of
 *       cvSVD (the PnPsolver rows) and is not pinned to OpenCV 2.4.9: a 4-point hypothesis depends on the
 *       null-space basis the SVD happens to produce (section 5), so the device is pinned to tests/pnp_reference.py byte for byte.
 * Inputs.  kps = mvKeysUn (pt and octave are read), camera = a pgorb_kf_pose of which fx, fy, cx, cy are read (invfx / invfy are
 * copied to pose_out), kp_point[i] = the table index of vpMapPointMatches[i] or -1, the table as above (pos is read), point_bad
 * [npoints] (NULL = none).  A correspondence is a keypoint whose slot is valid and not bad, in keypoint order (:78-101);
 * mvMaxError = mvLevelSigma2[octave]*th2 in float.
 *   params: SetRansacParameters' arguments (probability and epsilon are floats here; min_set must be 4) with th2, then the state a
 *       solver carries between calls: first_iteration = mnIterations, best_inliers_in = mnBestInliers (with best_inlier_in =
 *       mvbBestInliers by KEYPOINT and best_pose_in = mBestTcw; without both of them nothing is carried), and niterations.
 *       pgorb_pnp_ransac returns the adjusted mRansacMinInliers and mRansacMaxIts of one N (:133-152), made on the host: no
 *       device logarithm decides a ceil.
 *   The window.  iterate's loop condition is `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`, an OR: a call runs
 *       max(mRansacMaxIts - first_iteration, niterations) iterations unless Refine succeeds earlier.  draws [W][4] with W =
 *       max(max_iterations, niterations) = raw rand() values (below 2^31), row k for the call's k-th iteration; RandomInt's formula
 *       and the swap-with-back selection over mvAllIndices are applied here.  Every hypothesis of the window is evaluated; trace
 *       (may be NULL) [W] receives them (R, t in double, mnInliersi, flags = 1; zeros past the window).
 *   The stop rule (:209-238).  At an iteration with mnInliersi >= min: the best set is replaced only for mnInliersi >
 *       mnBestInliers; Refine() then runs on the BEST set and the call returns its pose only for refined > min (strict).
 * Outputs.  The return value is nInliers.  PGORB_PNP_FOUND | PGORB_PNP_REFINED: pose_out = Refine's R, t converted to float,
 * inlier = mvbRefinedInliers by keypoint.  PGORB_PNP_FOUND | PGORB_PNP_NO_MORE: mnIterations reached mRansacMaxIts with
 * mnBestInliers >= min: pose_out = mBestTcw, inlier = mvbBestInliers.  pose_out is a complete pgorb_kf_pose (Tcw, Ow = -Rcw.t()*tcw
 * as Frame::SetPose, the camera copied); kp_point_out[i] = kp_point[i] where inlier[i], else -1.  Without PGORB_PNP_FOUND: returns
 * 0, pose_out zeroed, inlier all 0, kp_point_out all -1.  PGORB_PNP_FEW (with NO_MORE): N < min, nothing evaluated, the carried
 * state untouched.  best_inlier_out / best_pose_out (may be NULL) = the state after the call.  info (may be NULL) = PGORB_PNP_INFO
 * int32: status bits, N, the adjusted min inliers, mRansacMaxIts, mnIterations after the call, nInliers, mnBestInliers, the
 * iteration returned (-1: none, or mBestTcw).
 * Determinism: a pair's result depends on its inputs only, not on its place in a batch, the batch size, the stream or a repeat; the
 * single call is a one-pair batch.  Every sum runs from 0 in index order (Refine's too), so the device equals the reference's
 * sequential form.
 * PGORB_E_ARG (single call, checked on the host first): a negative count, a NULL array that is read, min_set != 4 or another
 * parameter out of range, a slot outside [-1, npoints), the octave of a kept correspondence outside the context's levels, a value
 * that is not finite, a draw >= 2^31.  The batched form checks the parameters and the limits only: a bad index or octave counts as
 * no point.  PGORB_E_LIMIT: more than 16000 keypoints per frame; W above PGORB_PNP_MAX_WINDOW.
 *   pgorb_pnp_solver_batch_device: pair p solves frame d_pair_frame[p] (NULL: frame p) with the camera of that frame; d_kp_point,
 *       d_inlier, d_kp_point_out, d_best_inlier (in and out, NULL = nothing carried, nothing kept) [npairs][cap_per_frame]; d_best_pose
 *       (in and out, may be NULL), d_pose_out, d_ninliers [npairs]; d_first_iteration / d_best_inliers_in [npairs] (NULL = the params'
 *       values); d_draws [npairs][W][4], d_trace [npairs][W], d_info [npairs][PGORB_PNP_INFO].  Three launches; the records, the
 *       hypotheses and Refine's arrays live in the context's scratch arena (138 bytes per pair and keypoint, 104 per pair and
 *       iteration of W). */
typedef struct pgorb_pnp_params { float probability; int32_t min_inliers, max_iterations, min_set; float epsilon, th2;
                                  int32_t first_iteration, niterations, best_inliers_in; } pgorb_pnp_params;
typedef struct pgorb_pnp_hypothesis { double R[9], t[3]; int32_t inliers, flags; } pgorb_pnp_hypothesis;
#define PGORB_PNP_FEW      1   /* N < the adjusted min inliers: bNoMore, nothing evaluated */
#define PGORB_PNP_FOUND    2   /* a pose is returned */
#define PGORB_PNP_NO_MORE  4   /* bNoMore */
#define PGORB_PNP_REFINED  8   /* the pose is Refine's */
#define PGORB_PNP_INFO     8
#define PGORB_PNP_MAX_WINDOW 1024
int  pgorb_pnp_ransac(float probability, int min_inliers, int max_iterations, int min_set, float epsilon, int N,
        int32_t* min_inliers_out, int32_t* max_iterations_out);
int  pgorb_pnp_solver(pgorb_ctx* ctx, const pgorb_keypoint* kps, int n, const pgorb_kf_pose* camera, const int32_t* kp_point /*[n]*/,
        int npoints, const pgorb_map_point* points, const uint8_t* point_bad /*[npoints] or NULL*/,
        const pgorb_pnp_params* params, const uint32_t* draws /*[W][4]*/,
        const uint8_t* best_inlier_in /*[n] or NULL*/, const pgorb_kf_pose* best_pose_in /*or NULL*/,
        pgorb_kf_pose* pose_out, uint8_t* inlier /*[n]*/, int32_t* kp_point_out /*[n]*/,
        uint8_t* best_inlier_out /*[n] or NULL*/, pgorb_kf_pose* best_pose_out /*or NULL*/,
        pgorb_pnp_hypothesis* trace /*[W] or NULL*/, int32_t* info);
int  pgorb_pnp_solver_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_pair_frame, int npairs, const pgorb_kf_pose* d_camera, const int32_t* d_kp_point,
        int npoints, const pgorb_map_point* d_points, const uint8_t* d_point_bad, const pgorb_pnp_params* params /*host, one for all*/,
        const int32_t* d_first_iteration, const int32_t* d_best_inliers_in, const uint32_t* d_draws,
        uint8_t* d_best_inlier, pgorb_kf_pose* d_best_pose, pgorb_kf_pose* d_pose_out, uint8_t* d_inlier, int32_t* d_kp_point_out,
        pgorb_pnp_hypothesis* d_trace, int32_t* d_info, int32_t* d_ninliers, void* hip_stream);

/*   pgorb_initializer   Initializer::Initialize (src/Initializer.cc:33-929; Tracking::MonocularInitialization, src/Tracking.cc:564-631)
 *       with the constructive part of Tracking::CreateInitialMapMonocular (:633-680): the step between
 *       pgorb_search_for_initialization and the first pgorb_global_bundle_adjustment.  max_iterations sets of 8 matches, a homography
 *       and a fundamental matrix from each (the SAME set for both), each scored over all N matches; RH = SH/(SH + SF) picks the model
 *       (> 0.40: H); its 8 (H) or 4 (F) motion hypotheses are triangulated over the model's inliers and the reference's decision
 *       is taken.  It is this project's READING of cv::Mat arithmetic and of OpenCV 2.4.9's JacobiSVDImpl_<float>, completion loop
 *       included (DESIGN.md sections 4 and 5): an 8-point hypothesis depends on that routine to the last bit, so the device is
 *       pinned to tests/init_reference.py byte for byte; only the parallax (an acos) is compared with a tolerance.
 * Inputs.  kps1 / kps2: mvKeysUndistorted of the reference and the current frame (only pt is read; Normalize runs over ALL of
 * them).  camera: fx, fy, cx, cy are read (the whole record is copied into pose_out).  matches12[i1] = i2 or -1 (vMatches12, what
 * pgorb_search_for_initialization writes).  params: sigma and max_iterations (Tracking.cc:578 passes 1.0 and 200), min_parallax and
 * min_triangulated (Initializer.cc:116-118 pass 1.0 and 50).  draws [max_iterations][8]: raw rand() values in [0, 2^31); the
 * library applies RandomInt's formula and the swap-with-back selection over a fresh vAvailableIndices per iteration.
 * Outputs.  The return value is the number of triangulated matches, 0 when Initialize would return false.  pose_out[0] = the
 * identity pose of the reference frame, pose_out[1] = [R21 | t21], both complete records (Ow as Frame::SetPose, the camera
 * copied).  P3D [n1][3] = vP3D and triangulated [n1] = vbTriangulated (entries CheckRT never writes are zeros); matches12_out[i] =
 * matches12[i] where triangulated, else -1 (Tracking.cc:612-619).  On failure pose_out, P3D, triangulated are zeroed and
 * matches12_out is all -1; trace, info and finfo are still written.
 * The map (all seven NULL together, or none): one point per triangulated match in rising i1 order, points[k].pos = P3D[i1] with
 * the normal and the distances zero (pgorb_refresh_map_points fills them); kf_point1 [n1] / kf_point2 [n2] = the slot or -1;
 * obs_start [n1 + 1] (2*min(k, npoints)), obs_frame / obs_idx [2*n1] = (f1, i1) then (f2, i2) per point, -1 past the points (the
 * single call's frames are 0 and 1); *npoints.  This is what pgorb_refresh_map_points and pgorb_global_bundle_adjustment_device
 * read.  The median-depth rescale and its two acceptance tests (Tracking.cc:685-711) stay with the caller.
 * trace (may be NULL) [max_iterations]: every hypothesis.  info [PGORB_INIT_INFO] int32: [0] status bits, [1] N, [2] best iteration
 * of H or -1, [3] its inliers, [4] best iteration of F or -1, [5] its inliers, [6] the motion hypothesis the decision examined or
 * -1, [7..14] nGood of the 8 (4) hypotheses, [15] the chosen model's inlier count, [16] the return value.  finfo
 * [PGORB_INIT_FINFO] float: [0] SH, [1] SF, [2] RH, [3..10] the parallaxes.
 * Errors, single call, checked on the host first: PGORB_E_ARG (a negative count, a NULL array that is read or written, matches12
 * outside [-1, n2), a coordinate or camera value that is not finite, sigma <= 0, max_iterations < 1, a draw >= 2^31);
 * PGORB_E_LIMIT (more than 16000 keypoints in a frame, max_iterations > PGORB_INIT_MAX_ITERATIONS).
 *   pgorb_initializer_batch_device: pair p initialises from frames d_pair_f1[p] (reference) and d_pair_f2[p] (current) of one
 *       batch in the layout of pgorb_extract_batch_device, with the camera of frame d_pair_f1[p]; d_matches12 [npairs][cap] is
 *       what pgorb_search_for_initialization_batch_device writes; d_draws [npairs][max_iterations][8].  Outputs by pair:
 *       d_pose_out [npairs][2], d_P3D [npairs][cap][3], d_triangulated, d_matches12_out [npairs][cap], the map (d_points,
 *       d_kf_point1, d_kf_point2 [npairs][cap], d_obs_start [npairs][cap + 1], d_obs_frame, d_obs_idx [npairs][2*cap], d_npoints
 *       [npairs]; frame indices are the batch's), d_trace [npairs][max_iterations], d_info [npairs][PGORB_INIT_INFO] (the count
 *       is d_info[p][16]), d_finfo [npairs][PGORB_INIT_FINFO].  Checks the parameters and the limits only: a match index outside
 *       [0, n[f2]) counts as no match.  Three launches (k_init_prepare, k_init_hypotheses, k_init_reconstruct), no atomics; the
 *       scratch arena holds 40 + 136 bytes per (pair, keypoint slot) and 120 + cap/4 bytes per (pair, iteration). */
typedef struct pgorb_init_params { float sigma; int32_t max_iterations; float min_parallax; int32_t min_triangulated; } pgorb_init_params;
typedef struct pgorb_init_hypothesis { float H21[9], F21[9], scoreH, scoreF; int32_t inliersH, inliersF, set[8]; } pgorb_init_hypothesis;
#define PGORB_INIT_FEW           1   /* N < 8: nothing is evaluated (the reference would index an empty vector) */
#define PGORB_INIT_NO_MODEL      2   /* SH == 0 and SF == 0 */
#define PGORB_INIT_MODEL_H       4   /* RH > 0.40 */
#define PGORB_INIT_MODEL_F       8
#define PGORB_INIT_OK            16  /* Initialize returned true */
#define PGORB_INIT_DEGENERATE_H  32  /* d1/d2 < 1.00001 || d2/d3 < 1.00001 (:597) */
#define PGORB_INIT_AMBIGUOUS     64  /* nsimilar > 1 (:517); secondBestGood < 0.75*bestGood false (:721) */
#define PGORB_INIT_FEW_GOOD      128 /* maxGood < nMinGood (:517); either bestGood clause false (:721) */
#define PGORB_INIT_LOW_PARALLAX  256 /* the parallax clause */
#define PGORB_INIT_INFO          17
#define PGORB_INIT_FINFO         11
#define PGORB_INIT_MAX_ITERATIONS 1024
int  pgorb_initializer(pgorb_ctx* ctx, const pgorb_keypoint* kps1, int n1, const pgorb_keypoint* kps2, int n2,
        const pgorb_kf_pose* camera, const int32_t* matches12 /*[n1]*/, const pgorb_init_params* params,
        const uint32_t* draws /*[max_iterations][8]*/, pgorb_kf_pose* pose_out /*[2]*/, float* P3D /*[n1][3]*/,
        uint8_t* triangulated /*[n1]*/, int32_t* matches12_out /*[n1]*/,
        pgorb_map_point* points /*[n1]*/, int32_t* kf_point1 /*[n1]*/, int32_t* kf_point2 /*[n2]*/, int32_t* obs_start /*[n1 + 1]*/,
        int32_t* obs_frame /*[2*n1]*/, int32_t* obs_idx /*[2*n1]*/, int32_t* npoints,
        pgorb_init_hypothesis* trace /*[max_iterations] or NULL*/, int32_t* info, float* finfo);
int  pgorb_initializer_batch_device(pgorb_ctx* ctx, const pgorb_keypoint* d_kps, const int32_t* d_n, int cap_per_frame,
        const int32_t* d_pair_f1, const int32_t* d_pair_f2, int npairs, const pgorb_kf_pose* d_camera /*by frame*/,
        const int32_t* d_matches12, const pgorb_init_params* params /*host, one for all*/, const uint32_t* d_draws,
        pgorb_kf_pose* d_pose_out, float* d_P3D, uint8_t* d_triangulated, int32_t* d_matches12_out,
        pgorb_map_point* d_points, int32_t* d_kf_point1, int32_t* d_kf_point2, int32_t* d_obs_start, int32_t* d_obs_frame,
        int32_t* d_obs_idx, int32_t* d_npoints, pgorb_init_hypothesis* d_trace, int32_t* d_info, float* d_finfo, void* hip_stream);

/*   pgorb_local_bundle_adjustment  Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) (src/Optimizer.cc:453-778) with the g2o
 *       path under it (VertexSE3Expmap, VertexSBAPointXYZ, EdgeSE3ProjectXYZ with its ANALYTIC Jacobian, RobustKernelHuber,
 *       BlockSolver_6_3 with the Schur complement over the marginalised points, OptimizationAlgorithmLevenberg), monocular (mvuRight
 *       < 0), in double: the step of LocalMapping::Run after SearchInNeighbors.  It is this project's READING of g2o and Eigen
 *       (DESIGN.md sections 4 and 5 list the ten readings), anchored by the CPU tests of tests/test_local_bundle_adjustment.py and
 *       not pinned to a g2o build.
 * Inputs.  Key frames as for pgorb_refresh_map_points: nkf of them, each its undistorted keypoints (pt and octave are read), n[f], its
 * pgorb_kf_pose (Tcw, fx, fy, cx, cy are read), kf_bad[f] = pKF->isBad() (NULL = none), its slots kf_point[f][i] = the table index of
 * GetMapPoint(i) or -1, and kf_fixed_id0[f] != 0 for the key frame with mnId == 0 (setFixed(pKFi->mnId==0), :529; NULL = none).
 * The window: local_kf[nlocal] = pKF and GetVectorCovisibleKeyFrames() by index, in any order; the covisibility graph stays with the
 * caller.  Points: the resident table of pgorb_refresh_map_points -- pos (in and out), point_bad, and the observations as CSR of
 * (obs_frame, obs_idx).  Nothing else is passed; the library derives, as flags and so without an order:
 *   local key frames   the named key frames that are not bad.  (The reference keeps pKF itself in lLocalKeyFrames even when it is
 *                  bad, :458; here every named bad key frame is dropped, pKF included: do not adjust around a bad key frame.)
 *   local points   not bad and in a slot of a local key frame that is not bad (:470-486)              -> is_local [npoints]
 *   fixed cameras  not bad, observing a local point, not named by the window (:488-504)               -> role [nkf]: PGORB_LBA_ROLE_*
 *   edges          every CSR observation of a local point in a key frame that is not bad (:585-589)
 * rounds: 2 is the normal path; 1 is bDoMore == false (:662-709): no classification between the rounds and no second optimize.
 * The asynchronous pbStopFlag INSIDE g2o's loop is not reproducible and is not offered.
 * Outputs.  The return value is the number of erased observations (vToErase.size()).  pose_out [nkf]: for every local key frame a
 * complete pgorb_kf_pose (Converter::toCvMat(SE3Quat) to float, then SetPose's Ow = -Rcw.t()*tcw), the input's camera kept; the
 * single call copies the input for the others, the batched form leaves them alone.  points[].pos of the local points are
 * overwritten (Converter::toCvMat(Vector3d) to float); normal and distances keep their bytes -- pMP->UpdateNormalAndDepth() (:776)
 * is pgorb_refresh_map_points(_batch_device) with what = PGORB_MP_NORMAL_DEPTH over the local points, on the same arrays.
 * Per observation, aligned with the CSR: erase (membership of vToErase, :715-728), chi2 (float; what e->chi2() read at the last
 * classification, stale where the reference's is: readings 6 and 7) and level (1 = set aside after the first optimize, :680-683);
 * all 0 where the observation is no edge.  info (may be NULL) = PGORB_LBA_INFO int32: status bits, edges, local points, local key
 * frames, fixed key frames, iterations and Levenberg trials of the first optimize, the same of the second, edges set to level 1.
 * PGORB_LBA_NOTHING: no edge (no local point, or none observed in a live key frame) -- nothing is optimised, returns 0, pose_out of
 * the local key frames = the input byte for byte, the points keep their bytes.
 * PGORB_LBA_NONFINITE: the active chi2 a Levenberg iteration starts from, or an edge's chi2 at a classification, is not finite --
 * returns 0, outputs as for PGORB_LBA_NOTHING, erase / chi2 / level 0, the counters of info 0.
 * Determinism: no floating-point atomics; every sum runs in one documented order (csrc/local_ba.hip: a point's edges in CSR order,
 * a camera's in table-then-CSR order, chi2 and computeScale in one fixed tree); a window's result depends on its inputs alone, not
 * on its place in a batch, the stream or a repeat; the single call equals the batched one byte for byte.
 * PGORB_E_ARG (single call, on the host before anything else): a negative count, a NULL array that is read or written, rounds
 * outside 1..2, a local key frame, slot or observation out of range, obs_start not rising from 0, a key frame twice in one list, the
 * octave of an observed keypoint outside the context's levels, a value of Tcw, fx, fy, cx, cy or a point that is not finite, fx or
 * fy zero.  PGORB_E_LIMIT: more than 16000 keypoints in a key frame, or a window past a capacity below; the single call counts them
 * on the host.  The reduced camera system ((6 * local)^2 doubles a window) and the records (320 bytes an observation, 244 a point)
 * live in the context's scratch arena.  THE RECORDS ARE ADDRESSED BY CSR POSITION AND TABLE INDEX, so the arena, the clearing of
 * the flags and the zeroing of erase / chi2 / level scale with the WHOLE table passed (320 * nobs + 244 * npoints bytes, plus
 * 6 * nwin * nobs bytes of outputs), not with what the windows touch: pass the part of the map the windows can reach.
 *   Batched: the key frames are nframes frames of one batch (d_kps [nframes][cap_per_frame], d_n, d_pose, d_kf_bad, d_kf_fixed_id0
 *       [nframes], d_kf_point [nframes][cap_per_frame]); window w names d_win_kf[d_win_start[w] .. d_win_start[w + 1]), nwin_kf = the
 *       length of d_win_kf.  d_erase, d_chi2, d_level are [nwin][nobs], d_is_local [nwin][npoints], d_role [nwin][nframes], d_info
 *       [nwin][PGORB_LBA_INFO], d_nerased [nwin] (may be NULL); d_pose_out [nframes] is written for local key frames only and must
 *       not be d_pose.  THE RULE: points are updated in place, so two windows of one call must not share a local point (a key frame
 *       may be fixed in one and local in another: the input poses are read).  Nothing checks it; windows that break it stay inside
 *       the arrays and return garbage.  This form checks pointers, rounds and cap_per_frame only: an index out of range is no slot,
 *       no observation or no key frame, and a window past a capacity ends with PGORB_LBA_LIMIT in its status, nothing optimised,
 *       its points untouched.  Two launches, one workgroup per window. */
#define PGORB_LBA_NOTHING        1
#define PGORB_LBA_NONFINITE      2
#define PGORB_LBA_LIMIT          4
#define PGORB_LBA_INFO           10
#define PGORB_LBA_ROLE_NONE      0
#define PGORB_LBA_ROLE_LOCAL     1
#define PGORB_LBA_ROLE_FIXED     2
#define PGORB_LBA_MAX_LOCAL_KF   64
#define PGORB_LBA_MAX_FIXED_KF   256
#define PGORB_LBA_MAX_POINTS     8192
#define PGORB_LBA_MAX_EDGES      65536
int  pgorb_local_bundle_adjustment(pgorb_ctx* ctx,
        int nkf, const pgorb_keypoint* const* kps, const int32_t* n /*[nkf]*/, const pgorb_kf_pose* pose /*[nkf]*/,
        const uint8_t* kf_bad /*[nkf] or NULL*/, const int32_t* const* kf_point /*[nkf][n[f]]*/, const uint8_t* kf_fixed_id0 /*[nkf] or NULL*/,
        int nlocal, const int32_t* local_kf /*[nlocal]*/,
        int npoints, pgorb_map_point* points /*in and out: pos*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, const int32_t* obs_idx, int rounds,
        pgorb_kf_pose* pose_out /*[nkf]*/, uint8_t* erase, float* chi2, uint8_t* level /*[nobs]*/, uint8_t* is_local /*[npoints]*/,
        uint8_t* role /*[nkf]*/, int32_t* info);
int  pgorb_local_bundle_adjustment_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap_per_frame, const pgorb_kf_pose* d_pose,
        const uint8_t* d_kf_bad, const int32_t* d_kf_point, const uint8_t* d_kf_fixed_id0,
        const int32_t* d_win_start, const int32_t* d_win_kf, int nwin, int nwin_kf,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        const int32_t* d_obs_idx, int nobs, int rounds,
        pgorb_kf_pose* d_pose_out, uint8_t* d_erase, float* d_chi2, uint8_t* d_level, uint8_t* d_is_local, uint8_t* d_role,
        int32_t* d_info, int32_t* d_nerased, void* hip_stream);

/*   pgorb_optimize_essential_graph  Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
 *       LoopConnections, bFixScale) (src/Optimizer.cc:781-1044) with the g2o path under it (VertexSim3Expmap, EdgeSim3 with
 *       BaseBinaryEdge's NUMERIC Jacobian, BlockSolver_7_3 without a Schur complement, OptimizationAlgorithmLevenberg with
 *       setUserLambdaInit(1e-16)), in double: the call of LoopClosing::CorrectLoop (src/LoopClosing.cc:569) after SearchAndFuse.  One
 *       graph per call, spread over many workgroups.  It is this project's READING of g2o and Eigen (DESIGN.md sections 4 and 5),
 *       anchored by the CPU tests of tests/test_optimize_essential_graph.py and not pinned to a g2o build; LinearSolverEigen's
 *       SimplicialLDLT is read as a Cholesky L L' in index order, stored as a block skyline.
 * Inputs.  nkf key frames in strictly rising mnId order (kf_id; index order is then vertex-id order, g2o's order), pose (Tcw is read,
 * the camera is copied through), kf_bad (NULL = none), loop_kf and cur_kf by index, fix_scale.  has_corrected / corrected =
 * CorrectedSim3, has_non_corrected / non_corrected = NonCorrectedSim3 (pgorb_sim3d in double, as the reference's maps hold them; the
 * flag arrays may be NULL = empty map).  Four candidate lists by index, holding what the containers hold, not what survives:
 *   loop_conn [nloop_conn][3] = (i, j, pKF_i->GetWeight(pKF_j)) in LoopConnections' map-then-set iteration order;
 *   parent [nkf] = GetParent() or -1;  loop_edge_start [nkf + 1] / loop_edge = GetLoopEdges() per key frame as CSR;
 *   covis_start [nkf + 1] / covis / covis_weight = the covisibles per key frame as CSR, with weights.
 * min_feat is the reference's 100, iterations its 20.  The point table of pgorb_refresh_map_points: pos (in and out), point_bad, and
 * point_ref_kf [npoints] = the index of the key frame :1020-1029 selects (mnCorrectedByKF == cur ? mnCorrectedReference :
 * GetReferenceKeyFrame()), -1 = none.
 * Derived on the device.  The vertices (:809-844: the corrected estimate where present, else Sim3(Rcw, tcw, 1) of the float pose;
 * loop_kf fixed).  The edges, kind 0..3: loop connections (:852-880: weight < min_feat skips unless (i, j) == (cur, loop); they make
 * sInsertedEdges), then per key frame the spanning-tree edge to parent (1), the loop edges with a smaller mnId (2), and the
 * covisibles (3) with weight >= min_feat that are not parent, not a child (parent[n] == i), not a loop edge of i, not bad, of a
 * smaller mnId and not in sInsertedEdges.  Measurements: vScw on both sides for kind 0, NonCorrectedSim3 where present else vScw
 * for the others.  The edge order -- kind 0 in list order, then per key frame 1, 2, 3 -- is the order every per-vertex sum runs in.
 * ONE DEPARTURE: a bad key frame gets no vertex, no edge and no output (the reference would dereference a null vertex at :998;
 * GetAllKeyFrames() never returns one).  A key frame with no surviving edge is not in the system and keeps its pose.
 * Outputs.  The return value is the number of optimised (free, active) vertices.  sim3_out [nkf] = the recovered estimates (zeros for
 * a bad key frame).  pose_out [nkf]: for a key frame with an edge [R | t/s] through Converter::toCvSE3 to float, then SetPose's Ow,
 * the camera kept; the input's bytes for the others.  points[].pos is overwritten for every point that is not bad and whose
 * point_ref_kf is valid and not bad with correctedSwr.map(Srw.map(pos)) in double, rounded to float; other points, normal and the
 * distances keep their bytes -- pgorb_refresh_map_points_batch_device with PGORB_MP_NORMAL_DEPTH follows on the same arrays.
 * edge_out (may be NULL; room for nloop_conn + nkf + loop edges + covisibles records) = the derived edges with e->chi2() at the
 * final estimates.  info (may be NULL) = PGORB_EG_INFO int32: status bits, vertices, free vertices, edges of kind 0, 1, 2, 3,
 * iterations, Levenberg trials, envelope blocks.
 * PGORB_EG_NOTHING: no edge, or every active vertex fixed -- returns 0, pose_out = pose byte for byte, sim3_out = the input
 * estimates, the points untouched.  PGORB_EG_NONFINITE: the chi2 a Levenberg iteration starts from is not finite -- the same
 * outputs.  PGORB_EG_LIMIT: the envelope exceeds PGORB_EG_MAX_ENVELOPE_BLOCKS -- the same outputs; the single call then returns
 * PGORB_E_LIMIT.
 * Determinism: no floating-point atomics; a vertex's sums run in edge order, chi2 and computeScale in one fixed tree; the result
 * depends on the inputs alone, not on the stream, a repeat or what the context ran before; the single call equals the device form
 * byte for byte.
 * PGORB_E_ARG (single call, on the host before anything else): a negative count, a NULL array that is read or written, kf_id not
 * strictly rising, loop_kf, cur_kf, a list entry, a parent or point_ref_kf out of range, an edge from a key frame to itself, a start
 * array not rising from 0, iterations < 0, a value of Tcw, a Sim3 that is read or a point that is not finite, a scale <= 0.
 * PGORB_E_LIMIT: nkf > PGORB_EG_MAX_KF, or nloop_conn + nkf + loop edges + covisibles > PGORB_EG_MAX_EDGES (the candidates bound
 * the edges).  The device form checks pointers and these two limits only: a list entry out of range is no candidate.  The scratch
 * arena holds 336 bytes per key frame, 1456 per candidate and 788 per envelope block (the skyline and its factor).  THE ENVELOPE IS
 * KNOWN ON THE DEVICE ONLY, so the arena is sized for min(PGORB_EG_MAX_ENVELOPE_BLOCKS, nkf (nkf + 1) / 2) blocks whatever the graph
 * needs -- 103 MB from 512 key frames on, where a ride-shaped graph of 500 key frames uses 3225 blocks (2.5 MB) -- and for every
 * candidate, and the context keeps it until it is destroyed.
 *   pgorb_optimize_essential_graph_device: asynchronous on hip_stream; nloop_edges and ncovis are the lengths of the two CSR value
 *       arrays; returns 0 and leaves the count in d_info[2], so d_info is required.  d_pose_out must not be d_pose.  Launches:
 *       k_eg_prepare, iterations x (k_eg_linearize, k_eg_assemble, k_eg_step), k_eg_finish; no host round trip, no cooperative
 *       launch; a kernel of a stopped graph returns at once. */
typedef struct pgorb_sim3d { double r[4] /* x y z w, not renormalised */, t[3], s; } pgorb_sim3d;   /* g2o::Sim3 (pgorb_sim3 is the matchers' float record) */
typedef struct pgorb_eg_edge { int32_t i, j, kind, pad; double chi2; } pgorb_eg_edge;         /* vertex 0, vertex 1 */
#define PGORB_EG_NOTHING        1
#define PGORB_EG_NONFINITE      2
#define PGORB_EG_LIMIT          4
#define PGORB_EG_INFO           10
#define PGORB_EG_MAX_KF         2048
#define PGORB_EG_MAX_EDGES      65536
#define PGORB_EG_MAX_ENVELOPE_BLOCKS 131072
int  pgorb_optimize_essential_graph(pgorb_ctx* ctx,
        int nkf, const uint64_t* kf_id /*[nkf]*/, const pgorb_kf_pose* pose /*[nkf]*/, const uint8_t* kf_bad /*[nkf] or NULL*/,
        int loop_kf, int cur_kf, int fix_scale,
        const uint8_t* has_corrected /*[nkf] or NULL*/, const pgorb_sim3d* corrected /*[nkf]*/,
        const uint8_t* has_non_corrected /*[nkf] or NULL*/, const pgorb_sim3d* non_corrected /*[nkf]*/,
        int nloop_conn, const int32_t* loop_conn /*[nloop_conn][3]*/, const int32_t* parent /*[nkf]*/,
        const int32_t* loop_edge_start /*[nkf + 1]*/, const int32_t* loop_edge,
        const int32_t* covis_start /*[nkf + 1]*/, const int32_t* covis, const int32_t* covis_weight,
        int min_feat, int iterations,
        int npoints, pgorb_map_point* points /*in and out: pos*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        const int32_t* point_ref_kf /*[npoints]*/,
        pgorb_sim3d* sim3_out /*[nkf]*/, pgorb_kf_pose* pose_out /*[nkf]*/, pgorb_eg_edge* edge_out /*or NULL*/, int32_t* info);
int  pgorb_optimize_essential_graph_device(pgorb_ctx* ctx,
        int nkf, const uint64_t* d_kf_id, const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad,
        int loop_kf, int cur_kf, int fix_scale,
        const uint8_t* d_has_corrected, const pgorb_sim3d* d_corrected,
        const uint8_t* d_has_non_corrected, const pgorb_sim3d* d_non_corrected,
        int nloop_conn, const int32_t* d_loop_conn, const int32_t* d_parent,
        const int32_t* d_loop_edge_start, const int32_t* d_loop_edge, int nloop_edges,
        const int32_t* d_covis_start, const int32_t* d_covis, const int32_t* d_covis_weight, int ncovis,
        int min_feat, int iterations,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_point_ref_kf,
        pgorb_sim3d* d_sim3_out, pgorb_kf_pose* d_pose_out, pgorb_eg_edge* d_edge_out, int32_t* d_info, void* hip_stream);

/*   pgorb_global_bundle_adjustment  Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag, nLoopKF, bRobust), that is
 *       Optimizer::BundleAdjustment over every key frame and map point (src/Optimizer.cc:41-46, :49-237), with the g2o path under it
 *       (VertexSE3Expmap, VertexSBAPointXYZ, EdgeSE3ProjectXYZ with its ANALYTIC Jacobian, optional RobustKernelHuber, BlockSolver_6_3
 *       with the Schur complement over the marginalised points, OptimizationAlgorithmLevenberg), monocular (mvuRight < 0), in double:
 *       the call of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:648-752) and of Tracking::CreateInitialMapMonocular
 *       (src/Tracking.cc:682).  One problem per call, spread over many workgroups.  It is this project's READING of g2o and Eigen
 *       (DESIGN.md sections 4 and 5: the local-bundle-adjustment readings hold, the global rows add to them), anchored by the CPU
 *       tests of tests/test_global_bundle_adjustment.py and not pinned to a g2o build; LinearSolverEigen is read, as for the essential
 *       graph, as a Cholesky L L' in index order on a block skyline.
 * Inputs.  nkf key frames IN RISING mnId ORDER (index order is then vertex-id order, g2o's order), each its undistorted keypoints
 * (pt and octave are read), n[f], its pgorb_kf_pose (Tcw, fx, fy, cx, cy are read), kf_bad[f] = isBad() (NULL = none),
 * kf_fixed_id0[f] != 0 for the key frame with mnId == 0 (setFixed(pKF->mnId==0), :79; NULL = none: no gauge is fixed).  The point
 * table of pgorb_refresh_map_points: points (pos), point_bad, and the observations as CSR of (obs_frame, obs_idx).  iterations:
 * the reference's 10 from loop closing, 20 from initialisation.  robust: 0 from both callers; 1 = RobustKernelHuber with the
 * reference's const float thHuber2D = sqrt(5.99) -- a float, and 5.99, NOT local bundle adjustment's sqrt(5.991).  No kf_point
 * slots: the edges come from the observations alone.  Derived on the device, as flags and so without an order:
 *   vertices   every key frame that is not bad (:71-83); the fixed one is kf_fixed_id0.  (ONE DEPARTURE: the reference adds bad
 *              key frames' observations nowhere either (:105), but would hand a bad key frame in vpKFs no vertex and still read it
 *              at :193; GetAllKeyFrames() never returns one.  Here a bad key frame gets no vertex and its input bytes.)
 *   edges      every CSR observation of a point that is not bad, in a key frame that is not bad (:105-110)
 *   points     included when they have at least one edge (vbNotIncludedMP, :175-183)
 * One optimize(iterations): no classification, no second round, no erased observation.
 * Outputs.  The return value is the number of free active vertices (optimised key frames).  pose_out [nkf]: for EVERY key frame that
 * is not bad -- the fixed one and one without an edge included -- a complete pgorb_kf_pose: Converter::toCvMat(vSE3->estimate()) to
 * float (:193-210; for a vertex that did not move that is the round trip of the input through the quaternion, not the input's
 * bytes), then SetPose's Ow = -Rcw.t()*tcw, the camera kept; a bad key frame gets the input's bytes.  pos_out [npoints][3] (float):
 * Converter::toCvMat(Vector3d) for included points, the input position for the others.  kf_done [nkf], point_done [npoints]
 * (uint8): what mnBAGlobalForKF = nLoopKF marks (:196-209, :215-234): not bad, and for points also included.  in_place != 0 is the
 * nLoopKF == 0 branch (:202, :226): points[].pos of the done points is overwritten too; normal and the distances keep their bytes and
 * pgorb_refresh_map_points(_batch_device) with PGORB_MP_NORMAL_DEPTH follows on the same arrays, as after local bundle adjustment
 * (SetPose is the caller's copy of pose_out).  With in_place == 0 the table is not written.  chi2 [nobs] (float, may be NULL): each
 * edge's e->chi2() at the final estimates, 0 where the observation is no edge.  info (may be NULL) = PGORB_GBA_INFO int32: status
 * bits, edges, included points, vertices, free active vertices, iterations, Levenberg trials, envelope blocks.
 * PGORB_GBA_NOTHING: no edge, or no free active vertex (the reference would still move the points around fixed cameras; here
 * nothing is optimised) -- returns 0, pose_out is still the round trip above, pos_out the input, the table untouched, chi2 0.
 * PGORB_GBA_NONFINITE: the chi2 an iteration starts from is not finite -- the same outputs, the counters of info 0.
 * PGORB_GBA_LIMIT: the envelope exceeds PGORB_GBA_MAX_ENVELOPE_BLOCKS -- the same outputs, nothing is factorised; the single call
 * then returns PGORB_E_LIMIT.  The done flags do not depend on the status.
 * Determinism: no floating-point atomics; a point's sums run in CSR order, a camera's over the points in table order and a point's
 * edges in CSR order, chi2 and computeScale as per-workgroup trees whose partials are summed in one fixed tree; the result depends
 * on the inputs alone, not on the stream, a repeat or what the context ran before; the single call equals the device form byte
 * for byte.
 * PGORB_E_ARG (single call, on the host before anything else): a negative count, a NULL array that is read or written,
 * iterations < 0, an observation out of range, obs_start not rising from 0, a key frame twice in one list, the octave of an observed
 * keypoint outside the context's levels, a value of Tcw, fx, fy, cx, cy or a point that is not finite, fx or fy zero.
 * PGORB_E_LIMIT: nkf > PGORB_GBA_MAX_KF, npoints > PGORB_GBA_MAX_POINTS, observations > PGORB_GBA_MAX_EDGES (each from the counts
 * alone), more than 16000 keypoints in a key frame.  The scratch arena holds 1636 bytes per key frame, 148 per point, 180 per
 * observation and 292 per envelope block.  THE RECORDS ARE ADDRESSED BY TABLE INDEX AND CSR POSITION, so the arena scales with the
 * table passed, and THE ENVELOPE IS KNOWN ON THE DEVICE ONLY, so it is sized for min(PGORB_GBA_MAX_ENVELOPE_BLOCKS, nkf (nkf + 1) / 2)
 * blocks whatever the map needs (38 MB from 512 key frames on); the context keeps it until it is destroyed.
 *   pgorb_global_bundle_adjustment_device: asynchronous on hip_stream; the key frames are nframes frames of one batch (d_kps
 *       [nframes][cap_per_frame], d_n, d_pose, d_kf_bad, d_kf_fixed_id0 [nframes]); nobs = the length of d_obs_frame / d_obs_idx.
 *       Returns 0 and leaves the count in d_info[4], so d_info is required.  d_pose_out must not be d_pose.  It checks pointers,
 *       iterations, cap_per_frame and the three count limits only: an index out of range is no observation.  Launches: k_gba_prepare,
 *       iterations x (k_gba_linearize, k_gba_begin, 10 x (k_gba_schur, k_gba_solve, k_gba_try, k_gba_decide)), k_gba_finish --
 *       42 * iterations + 2, so 842 at 20 iterations; no host round trip, no cooperative launch, no workgroup waits on another; a
 *       kernel behind the stop flag or the end of its iteration returns at once (about 4 us each: under 4 ms at 20 iterations). */
#define PGORB_GBA_NOTHING        1
#define PGORB_GBA_NONFINITE      2
#define PGORB_GBA_LIMIT          4
#define PGORB_GBA_INFO           8
#define PGORB_GBA_MAX_KF         2048
#define PGORB_GBA_MAX_POINTS     262144
#define PGORB_GBA_MAX_EDGES      2097152
#define PGORB_GBA_MAX_ENVELOPE_BLOCKS 131072
int  pgorb_global_bundle_adjustment(pgorb_ctx* ctx,
        int nkf, const pgorb_keypoint* const* kps, const int32_t* n /*[nkf]*/, const pgorb_kf_pose* pose /*[nkf]*/,
        const uint8_t* kf_bad /*[nkf] or NULL*/, const uint8_t* kf_fixed_id0 /*[nkf] or NULL*/,
        int npoints, pgorb_map_point* points /*pos; written when in_place*/, const uint8_t* point_bad /*[npoints] or NULL*/,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, const int32_t* obs_idx,
        int iterations, int robust, int in_place,
        pgorb_kf_pose* pose_out /*[nkf]*/, float* pos_out /*[npoints][3]*/, uint8_t* kf_done /*[nkf]*/, uint8_t* point_done /*[npoints]*/,
        float* chi2 /*[nobs] or NULL*/, int32_t* info);
int  pgorb_global_bundle_adjustment_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap_per_frame, const pgorb_kf_pose* d_pose,
        const uint8_t* d_kf_bad, const uint8_t* d_kf_fixed_id0,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        const int32_t* d_obs_idx, int nobs, int iterations, int robust, int in_place,
        pgorb_kf_pose* d_pose_out, float* d_pos_out, uint8_t* d_kf_done, uint8_t* d_point_done, float* d_chi2, int32_t* d_info,
        void* hip_stream);

/* ---- Map-point refresh: the distinctive descriptor and the normal / depth range of many points --------------------------
 *   pgorb_refresh_map_points   for every selected point what MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:259-324)
 *       followed by MapPoint::UpdateNormalAndDepth (:347-388) would store, exactly.  The reference runs the pair once per point at
 *       the end of CreateNewMapPoints (src/LocalMapping.cc:444-446), for every point of the new key frame after SearchInNeighbors'
 *       two Fuse rounds (:519-532), in ProcessNewKeyFrame (:152-153), in Tracking (Tracking.cc:533-534, :664-665, :1108-1109) and,
 *       one of the two only, after bundle adjustment and loop closing (Optimizer.cc:776, LoopClosing.cc:500, :534): `what`.
 *   Key frames: nkf of them, each its undistorted keypoints (mvKeysUn; only `octave` is read), descriptors, n[f], its
 *   pgorb_kf_pose (only Ow is read) and kf_bad[f] = pKF->isBad() (NULL = none).  Points: a table as pgorb_fuse's -- pose fields,
 *   32-byte descriptor, bad flag (NULL = none) -- with the observations as CSR of (obs_frame, obs_idx) = (index of the key frame
 *   in this call's list, keypoint index), and ref_obs[p] = the position of mpRefKF inside point p's own list.
 *   THE LIST ORDER IS THE CONTRACT: it must be the order the caller's mObservations iterates, a std::map<KeyFrame*, size_t>,
 *   i.e. key-frame ADDRESS order, which the library cannot know.  The first row with the smallest median wins and the normal is
 *   a float sum in that order, so another order is another result.
 *   ComputeDistinctiveDescriptors: a bad point or an empty list changes nothing.  The candidates are the observations whose key
 *   frame is not bad, in list order (:278-284); none -> nothing changes.  Distances[i][j] = DescriptorDistance; per row the
 *   median is sorted_row[(int)(0.5*(N-1))] (N = 4: index 1; N <= 2: the row's own 0, so the first candidate wins and no distance
 *   is computed); the first row with the strictly smallest median wins (median < BestMedian, :313).  Out: the 32 descriptor bytes
 *   and best_obs = the winner's position in the point's FULL list (bad key frames counted), -1 when nothing changed.
 *   UpdateNormalAndDepth: a bad point or an empty list changes nothing; bad key frames are NOT skipped (:367-374).  normal = the
 *   running float sum from 0, in list order, of normali/cv::norm(normali), normali = mWorldPos - Ow_i, then normal/n; dist =
 *   cv::norm(Pos - Ow_ref), level = the octave of the reference key frame's keypoint, mfMaxDistance = dist*mvScaleFactors[level],
 *   mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1] with the context's tables, under the OpenCV 2.4.9 readings of
 *   DESIGN.md section 4 (cv::norm in double, each term normali*(float)(1/norm) in float, float adds, normal*(float)(1.0/n)).
 *   status[q] (q = position in `select`): bit 0 (PGORB_MP_DESCRIPTOR) = the descriptor was written, bit 1 (PGORB_MP_NORMAL_DEPTH)
 *   = normal, min_distance, max_distance were written; PGORB_MP_LIMIT when the list of a live point is longer than
 *   PGORB_MP_MAX_OBS (the reference's only limit is its stack, float Distances[N][N], :292): nothing is written for that point,
 *   whatever `what` is.  Points that are not selected, and fields that are not written, keep their bytes.
 *   select[nsel] = table indices (NULL = every point, nsel = npoints); best_obs may be NULL; ref_obs may be NULL when what =
 *   PGORB_MP_DESCRIPTOR.  Returns the number of selected points with a positive status, or PGORB_E_ARG (an observation's key
 *   frame or keypoint out of range, obs_start not rising from 0, a key frame twice in one list, ref_obs outside the list of a
 *   live non-empty point that gets a normal / depth update, a selection index out of range or repeated, what outside 1..3) /
 *   PGORB_E_LIMIT (more than 16000 keypoints in a key frame). */
#define PGORB_MP_MAX_OBS 512
#define PGORB_MP_DESCRIPTOR 1
#define PGORB_MP_NORMAL_DEPTH 2
#define PGORB_MP_BOTH 3
#define PGORB_MP_LIMIT (-6)
#define PGORB_MP_BAD_INDEX (-1)
int  pgorb_refresh_map_points(pgorb_ctx* ctx,
        int nkf, const pgorb_keypoint* const* kps, const uint8_t* const* desc, const int32_t* n /*[nkf]*/,
        const pgorb_kf_pose* pose /*[nkf]*/, const uint8_t* kf_bad /*[nkf] or NULL*/,
        int npoints, pgorb_map_point* points /*in: pos; out: normal, distances*/, uint8_t* point_desc /*[npoints][32] in/out*/,
        const uint8_t* point_bad /*[npoints] or NULL*/, const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame,
        const int32_t* obs_idx, const int32_t* ref_obs /*[npoints]*/, int nsel, const int32_t* select /*[nsel] or NULL*/, int what,
        int32_t* best_obs /*[nsel] or NULL*/, int32_t* status /*[nsel]*/);
/* Batched, resident, asynchronous: the key frames are nframes frames of one batch in the layout of pgorb_extract_batch_device
 * (d_kps / d_desc [nframes][cap_per_frame], d_n [nframes]), d_pose and d_kf_bad [nframes]; the table and the lists as above, on
 * the device, nobs = the length of d_obs_frame / d_obs_idx.  This form does not check its inputs: a selection index outside the
 * table, an obs_start pair outside [0, nobs], an observation outside the batch or a ref_obs outside its list makes THAT point a
 * no-op with status PGORB_MP_BAD_INDEX, never an access out of bounds; a key frame listed twice and a point selected twice are
 * not detected (the latter writes the same bytes twice).  Points are independent, so one call may refresh any subset.
 * k_mp_bin bins the selection by list length, k_mp_seg<2 | 8 | 32 | 64> run 32 | 8 | 2 | 1 points per wave, k_mp_big one
 * workgroup per longer list (csrc/map_point.hip). */
int  pgorb_refresh_map_points_batch_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, int nframes, int cap_per_frame,
        const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, int npoints, pgorb_map_point* d_points, uint8_t* d_point_desc,
        const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
        const int32_t* d_ref_obs, int nsel, const int32_t* d_select, int what, int32_t* d_best_obs, int32_t* d_status,
        void* hip_stream);

/* ---- The covisibility graph: UpdateConnections, its views, and Tracking::UpdateLocalMap (csrc/covisibility.hip) --------------
 * The graph lives next to the map-point table, in the layouts the other entry points read.  Integers only; every result is exact.
 * Shared conventions.  Key frames are the nframes frames of one resident batch; their slots are d_kf_point [nframes][cap_per_frame]
 * (the table index of GetMapPointMatches()[s] or -1) with d_n.  The table is that of pgorb_refresh_map_points: d_point_bad (NULL =
 * none) and the observations as CSR d_obs_start [npoints + 1] / d_obs_frame [nobs]; obs_idx is not read.  d_kf_order [nframes]
 * (NULL = index order) is the RANK OF EACH KEY FRAME'S ADDRESS, a permutation of 0 .. nframes-1: the reference iterates
 * std::map<KeyFrame*, ..> and std::set<KeyFrame*> and sorts pair<int, KeyFrame*>, so address order decides every tie, and the
 * library cannot know it -- the same contract as the list order of pgorb_refresh_map_points.  An index out of range is no slot, no
 * observation and no key frame; a key frame whose rank is out of range or named by a larger index too is no key frame.  The device
 * forms never read or write out of bounds.
 * The graph state, one row of capacity conn_cap per key frame, updated in place:
 *   d_conn_kf / d_conn_w [nframes][conn_cap] + d_nconn   mConnectedKeyFrameWeights in address order: EVERY counter, also those below
 *                                                        the threshold (mConnectedKeyFrameWeights = KFcounter, KeyFrame.cc:470)
 *   d_ord_kf / d_ord_w + d_nord                          mvpOrderedConnectedKeyFrames / mvOrderedWeights
 *   d_parent [nframes] (-1 = none), d_first_connection [nframes] (mbFirstConnection), d_kf_id0 [nframes] (NULL = none; mnId == 0)
 *
 *   pgorb_update_connections_batch_device   KeyFrame::UpdateConnections() (src/KeyFrame.cc:392-482, with AddConnection and
 *       UpdateBestCovisibles, :226-260) of the key frames d_list [nlist] (distinct) ONE AFTER ANOTHER IN LIST ORDER, from the state
 *       passed in.  th is the reference's 15.  Readings: a bad point is skipped; an observation by the key frame itself is skipped;
 *       a key frame's own badness is not looked at; two slots holding one point count twice; pKFmax is the first strict maximum in
 *       address order; both sorts end as descending (weight, address); an empty KFcounter returns before anything changes; the
 *       parent is front() of the new list when first_connection and not id0.  The sequence decomposes exactly,
 *       so a workgroup per list member counts (k_cov_count, LDS integer atomics) and a workgroup per row finishes (k_cov_finish).
 *       d_row_status [nframes] bits: PGORB_COVIS_UPDATED (the row was rewritten from its own counters), RESORTED (an AddConnection
 *       changed its map: the ordered list is the whole map, sub-threshold entries included), EMPTY (a list member with an empty
 *       counter), FALLBACK (no counter reached th: pKFmax alone), PARENT_SET; PGORB_COVIS_LIMIT alone: the row would hold more than
 *       conn_cap entries -- that key frame keeps ALL its input bytes (parent and first_connection too) and adds no loop connection;
 *       what it sends to other rows is unaffected.  A row with status 0 was not written.
 *       LoopConnections (src/LoopClosing.cc:548-566; d_loop_conn may be NULL with loop_conn_cap 0): per list member the keys of its
 *       map right after its own update, minus its ordered list just before that update (which earlier members may already have
 *       re-sorted), minus the list members, as d_loop_conn [loop_conn_cap][3] = (i, j, GetWeight) in map-then-set address order,
 *       padded with (-1, -1, 0), which pgorb_optimize_essential_graph_device reads as no candidate: nloop_conn = loop_conn_cap
 *       chains without a download.  d_info [PGORB_COVIS_INFO]: [0] PGORB_COVIS_LIMIT when there are more than loop_conn_cap (then
 *       every record is padding; never with a NULL d_loop_conn), [1] their number (also when no record is asked for), [2] the number
 *       of rows with PGORB_COVIS_LIMIT, [3] 0.  THE DEVICE FORM REQUIRES every input connection row in address order with no key
 *       frame twice, as this call leaves them: only the single call checks it.  Another row cannot read or write out of bounds,
 *       but a repeated key frame keeps either weight, and the loop records of a list member whose row is not rewritten (EMPTY,
 *       nothing changed) are taken by position from the row as given, so they can name the wrong (j, weight).
 *   pgorb_update_connections   the same from host buffers (kf_point[f] [n[f]]), checked: returns the number of rows with
 *       PGORB_COVIS_UPDATED, or PGORB_E_ARG for a negative count, a NULL array that is read or written, th < 1, a slot, observation,
 *       list entry, connection or parent out of range, obs_start not rising from 0, a key frame twice in one observation list or in
 *       the list, kf_order not a permutation, a row count outside [0, conn_cap], a connection row not in address order, an ordered
 *       entry that is not in its row's map.  It equals the device form byte for byte.
 *   pgorb_covisibility_views_device   three views of the ordered rows (k_cov_views, a wave per key frame): d_best [nframes][nbest]
 *       padded with -1 = GetBestCovisibilityKeyFrames(nbest) (:277-285), the d_neigh of place recognition at nbest = 10 (NULL =
 *       skip); the CSR d_covis_start [nframes + 1] / d_covis / d_covis_weight that pgorb_optimize_essential_graph_device reads, rows
 *       in ordered order (NULL d_covis_start = skip), more than ncovis_cap entries -> PGORB_COVIS_LIMIT in d_info[0] and every row
 *       empty, d_info[1] = the entries; d_by_weight [nframes] (NULL = skip) = the length of GetCovisiblesByWeight(w) (:287-302):
 *       upper_bound with weightComp finds the first weight BELOW w, so an equal weight is inside the prefix, and when no weight is
 *       below w the reference returns an EMPTY vector: 0.
 *   pgorb_update_local_map_batch_device   Tracking::UpdateLocalMap (src/Tracking.cc:1186-1321) of npairs frames: problem p is frame
 *       d_pair_frame[p] (NULL: frame p) of the batch with the slots d_kp_point [npairs][cap_per_frame] (d_n of that frame in use).
 *       It reads the table, d_kf_bad (NULL = none), the key frames' slots, d_ord_kf / d_nord, d_parent and d_kf_order, and follows
 *       UpdateLocalKeyFrames literally: (1) a bad point's slot is cleared (d_kp_point_out, may be NULL, reports it), every other
 *       point votes for every key frame of its list, bad key frames included, without a self-skip; (2) the voted key frames in
 *       address order, the bad ones skipped, the strict maximum kept as the reference key frame; (3) the expansion over the
 *       first-stage entries only, stopped when the list is longer than max_local (the reference's 80): per entry the first of its
 *       best nbest (10) neighbours that is neither bad nor marked, the first such child in address order (parent[c] == i), and the
 *       parent if unmarked -- NO bad test, and after pushing it the outer loop ENDS (the reference's break, :1310); (4)
 *       UpdateLocalPoints (:1196-1210): key frames in list order, slots in slot order, a point kept if it is not NULL, not yet taken
 *       for this frame and not bad.  With no vote the reference returns early (:1235) and walks its previous list: optional
 *       d_prev_local_kf [npairs][lkf_cap] / d_nprev serve that; without them the lists come out empty; PGORB_LOCALMAP_NO_VOTES
 *       either way, d_ref_kf -1.  If all voted key frames are bad the list is empty and d_ref_kf -1 (= keep).  Outputs: d_local_kf
 *       [npairs][lkf_cap] + d_nlocal_kf, d_ref_kf, d_queries [npairs][qcap] + d_nq -- exactly what
 *       pgorb_search_local_points_batch_device takes -- and d_status; PGORB_LOCALMAP_LIMIT: a list past its capacity, both counts 0.
 *       k_cov_local, a workgroup per frame: the votes are LDS atomics, the first stage a scan in address order, the point union a
 *       first-position key per (frame, table point) and a scan; only the expansion is a short sequential walk.
 *   pgorb_update_local_map   one frame from host buffers, checked as above (nprev -1 = no previous list); returns nq.
 * Limits (PGORB_E_LIMIT): nframes <= PGORB_COVIS_MAX_KF (the LDS counters are one int32 per key frame), conn_cap <=
 * PGORB_COVIS_MAX_CONN (a row is sorted in LDS), lkf_cap <= PGORB_COVIS_MAX_KF, qcap <= 16000, cap_per_frame <= 16000.  Scratch
 * arena: UpdateConnections nlist * nframes * 4 bytes (the dense counter rows) + nlist * conn_cap; UpdateLocalMap npairs * npoints * 4.
 * Determinism: a result depends on its inputs alone, not on the batch position, the stream or a repeat. */
#define PGORB_COVIS_MAX_KF     4096
#define PGORB_COVIS_MAX_CONN   2048
#define PGORB_COVIS_UPDATED    1
#define PGORB_COVIS_RESORTED   2
#define PGORB_COVIS_EMPTY      4
#define PGORB_COVIS_FALLBACK   8
#define PGORB_COVIS_PARENT_SET 16
#define PGORB_COVIS_LIMIT      32
#define PGORB_COVIS_INFO       4
#define PGORB_LOCALMAP_NO_VOTES 1
#define PGORB_LOCALMAP_LIMIT    2
int  pgorb_update_connections(pgorb_ctx* ctx,
        int nkf, const int32_t* const* kf_point, const int32_t* n /*[nkf]*/, int npoints, const uint8_t* point_bad /*[npoints] or NULL*/,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, const int32_t* kf_order /*[nkf] or NULL*/,
        const uint8_t* kf_id0 /*[nkf] or NULL*/, int nlist, const int32_t* list, int th,
        int conn_cap, int32_t* conn_kf, int32_t* conn_w /*[nkf][conn_cap]*/, int32_t* nconn, int32_t* ord_kf, int32_t* ord_w, int32_t* nord,
        int32_t* parent /*[nkf]*/, uint8_t* first_connection /*[nkf]*/, int32_t* row_status /*[nkf]*/,
        int loop_conn_cap, int32_t* loop_conn /*[loop_conn_cap][3] or NULL*/, int32_t* info /*[PGORB_COVIS_INFO]*/);
int  pgorb_update_connections_batch_device(pgorb_ctx* ctx,
        const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame,
        int npoints, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs,
        const int32_t* d_kf_order, const uint8_t* d_kf_id0, int nlist, const int32_t* d_list, int th,
        int conn_cap, int32_t* d_conn_kf, int32_t* d_conn_w, int32_t* d_nconn, int32_t* d_ord_kf, int32_t* d_ord_w, int32_t* d_nord,
        int32_t* d_parent, uint8_t* d_first_connection, int32_t* d_row_status,
        int loop_conn_cap, int32_t* d_loop_conn, int32_t* d_info, void* hip_stream);
int  pgorb_covisibility_views_device(pgorb_ctx* ctx,
        int nframes, int conn_cap, const int32_t* d_ord_kf, const int32_t* d_ord_w, const int32_t* d_nord,
        int nbest, int32_t* d_best, int ncovis_cap, int32_t* d_covis_start, int32_t* d_covis, int32_t* d_covis_weight,
        int w, int32_t* d_by_weight, int32_t* d_info /*[2]*/, void* hip_stream);
int  pgorb_update_local_map(pgorb_ctx* ctx,
        int nkf, const int32_t* const* kf_point, const int32_t* n /*[nkf]*/, const uint8_t* kf_bad /*[nkf] or NULL*/,
        const int32_t* kp_point /*[nkp]*/, int nkp, int npoints, const uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame,
        int conn_cap, const int32_t* ord_kf /*[nkf][conn_cap]*/, const int32_t* nord, const int32_t* parent, const int32_t* kf_order,
        int nbest, int max_local, int nprev, const int32_t* prev_local_kf,
        int32_t* kp_point_out /*[nkp] or NULL*/, int lkf_cap, int32_t* local_kf, int32_t* nlocal_kf, int32_t* ref_kf,
        int qcap, int32_t* queries, int32_t* nq, int32_t* status);
int  pgorb_update_local_map_batch_device(pgorb_ctx* ctx,
        const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, const uint8_t* d_kf_bad,
        const int32_t* d_pair_frame, int npairs, const int32_t* d_kp_point,
        int npoints, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs,
        int conn_cap, const int32_t* d_ord_kf, const int32_t* d_nord, const int32_t* d_parent, const int32_t* d_kf_order,
        int nbest, int max_local, int lkf_cap, const int32_t* d_prev_local_kf, const int32_t* d_nprev,
        int32_t* d_kp_point_out, int32_t* d_local_kf, int32_t* d_nlocal_kf, int32_t* d_ref_kf,
        int qcap, int32_t* d_queries, int32_t* d_nq, int32_t* d_status, void* hip_stream);

/* ---- The cullings: LocalMapping::MapPointCulling and KeyFrameCulling with the map surgery they trigger (csrc/culling.hip) ------
 * The conventions of the covisibility block hold: key frames are the nframes frames of one resident batch with their slots
 * d_kf_point [nframes][cap_per_frame] + d_n, the table is that of pgorb_refresh_map_points (d_point_bad, the CSR d_obs_start /
 * d_obs_frame / d_obs_idx), d_kf_order is the address rank, an index out of range is no slot, no observation and no key frame, and
 * the device forms never read or write out of bounds.  Integers only; every result is exact.  Here d_kf_point and d_point_bad are
 * in/out and must not be NULL.
 * Erased observations.  The CSR keeps its shape during a culling: d_obs_live [nobs] (uint8, in/out) masks it, and a dead
 * observation does not exist for any count or walk.  Observations() is the number of live entries of the list (the monocular
 * reading).  d_ref_obs [npoints] (in/out) is the position of mpRefKF in the point's own list, as pgorb_refresh_map_points reads it.
 *
 *   pgorb_compact_observations_device   a fresh CSR from the old one, the mask and d_ref_obs: d_obs_start_out [npoints + 1],
 *       d_obs_frame_out / d_obs_idx_out [room for nobs], the order inside each list kept; d_ref_obs_out = ref_obs re-based to the
 *       compacted list, -1 when it names no live entry (an empty list always); d_info[0] = the new length.  THE OUTPUTS MUST NOT
 *       ALIAS THE INPUTS; the device form cannot see an alias.  The other entry points read these outputs as they are, with the old
 *       nobs as the bound.  k_cull_compact_scan (one workgroup) + k_cull_compact_copy (a thread per point).
 *   pgorb_map_point_culling_device   LocalMapping::MapPointCulling (src/LocalMapping.cc:170-207) over d_recent [nrecent] = table
 *       indices in mlpRecentAddedMapPoints order (distinct).  Per point d_first_kf_id (mnFirstKFid), d_visible, d_found (int32);
 *       cur_kf_id = mpCurrentKeyFrame->mnId; th_obs is the reference's 2.  The four tests in the reference's order, d_action [nrecent]:
 *       PGORB_CULL_MP_WAS_BAD (already bad), FOUND_RATIO ((float)found / (float)visible, one correctly rounded division, < 0.25f; a
 *       zero `visible` follows IEEE: inf or NaN is not below), FEW_OBS ((int)cur_kf_id - (int)first_kf_id >= 2 and Observations() <=
 *       th_obs), AGED (that difference >= 3: it only leaves the list), else KEEP; an entry out of range is dropped with
 *       PGORB_CULL_MP_NONE.  FOUND_RATIO and FEW_OBS run MapPoint::SetBadFlag (src/MapPoint.cc:172-187): the bad flag is set, the slot
 *       kf_point[f][i] of every live observer becomes -1, all its observations die.  d_recent_out + d_nrecent_out = the surviving
 *       list (KEEP), order kept, entries past the count keep their bytes.  d_info [PGORB_CULL_INFO] = (0, survivors, points culled,
 *       0).  Map::EraseMapPoint stays with the caller, who reads d_action.  k_cull_points, a thread per entry.
 *   pgorb_keyframe_culling_device   LocalMapping::KeyFrameCulling (:634-698) with KeyFrame::SetBadFlag (src/KeyFrame.cc:556-648) and
 *       MapPoint::EraseObservation (src/MapPoint.cc:132-158); one problem per call.  Reads d_kps (only `octave`), d_kf_id0 (NULL =
 *       none), d_kf_not_erase (NULL = none; mbNotErase), cur_kf; in/out the slots, the table with d_point_bad / d_obs_live /
 *       d_ref_obs, d_kf_bad, d_kf_to_be_erased (NULL = not reported) and the graph state of the covisibility block.
 *       The list is cur_kf's ordered row AS IT STANDS WHEN THE CALL STARTS (:640 copies it); more than list_cap members ->
 *       PGORB_CULL_LIMIT in d_info[0], the length in d_info[1], and nothing else is written.  The members are evaluated one after
 *       another in list order, each against the state the earlier SetBadFlags left; d_record [list_cap][4] = (key frame, nMPs,
 *       nRedundantObservations, action), records past the list keep their bytes:
 *         PGORB_CULL_KF_NONE   a member out of range, counts -1;  PGORB_CULL_KF_ID0   mnId == 0, counts -1;
 *         otherwise the slots in order: an empty slot or a bad point is skipped, every other point adds one to nMPs, and it is
 *         redundant when Observations() > 3 and at least three live observers other than the member have a keypoint octave <= the
 *         slot's octave + 1.  The decision is (double)nRedundant > 0.9 * (double)nMPs.
 *         PGORB_CULL_KF_WAS_BAD   kf_bad was set: counted and recorded, nothing written (a second SetBadFlag finds nothing left);
 *         PGORB_CULL_KF_KEEP;  PGORB_CULL_KF_TO_BE_ERASED   redundant with not_erase: mbToBeErased and nothing else;
 *         PGORB_CULL_KF_CULLED   SetBadFlag runs to its end before the next member is looked at.
 *       SetBadFlag of A: (1) for every key of A's map in address order, EraseConnection(A) on that row if it holds A: the entry
 *       leaves the row's map and the ordered list becomes the WHOLE map, sub-threshold entries included, descending (weight, address)
 *       -- the reading of PGORB_COVIS_RESORTED; (2) for every non-empty slot of A, with no bad test, EraseObservation(A) if the list
 *       holds a live (A, .): it dies; if ref_obs named it, ref_obs becomes the first live entry in list order or -1; with two or
 *       fewer live observations left the point goes bad (the slots of its remaining observers -1, all observations dead, ref_obs
 *       kept); A's own slots keep their values; (3) A's two rows are emptied; (4) the spanning tree: the children are the c with
 *       parent[c] == A and kf_bad[c] == 0 in address order, the candidates start as {parent[A]}; repeatedly, over the children in
 *       address order and each child's current ordered list in list order, the entry that is a candidate with the first strictly
 *       largest GetWeight (the weight in the child's map, 0 when absent) gives that child its parent, and the child joins the
 *       candidates; every child left gets parent[A] (-1 = none); parent[A] itself keeps its value, for mTcp; (5) kf_bad[A] = 1.
 *       Row bytes: a rewritten row holds -1 / 0 from its new count up to its old count, entries beyond the old count keep their bytes.
 *       d_row_status [nframes] bits: PGORB_CULL_ROW_ERASED (lost an entry, re-sorted), ROW_CLEARED (the culled key frame),
 *       ROW_REPARENTED; a row with status 0 keeps every byte.  d_info = (0, list length, key frames culled, points that went bad).
 *       mTcp, Map::EraseKeyFrame and KeyFrameDatabase::erase stay with the caller, who reads d_record.  k_cull_eval counts every
 *       member from the input state, a workgroup each; k_cull_walk, ONE workgroup, walks the list, counts a member again only when a
 *       cull cleared one of its slots or claimed a point one of its slots holds (nothing else can change its counts), and does the
 *       surgery of a culled member with the row sorts in LDS; a point held in several slots of A is handled once.  THE DEVICE FORM REQUIRES connection rows in address
 *       order with no key frame twice and no key frame twice in one observation list; only the single call checks it.
 *   pgorb_map_point_culling / pgorb_keyframe_culling   the same from host buffers (kf_point[f] [n[f]], kps[f]), checked: return
 *       the number of points / key frames culled, or PGORB_E_ARG for a negative count, a NULL array that is read or written, a slot,
 *       observation (key frame or keypoint), recent entry, connection, parent or cur_kf out of range, obs_start not rising from 0, a
 *       key frame twice in one list, a recent point twice, kf_order not a permutation, a row count outside [0, conn_cap], a connection
 *       row not in address order, an ordered entry that is not in its row's map, ref_obs outside [-1, length) of a non-empty list,
 *       list_cap < 1.  They equal the device forms byte for byte.
 * Limits (PGORB_E_LIMIT): nframes <= PGORB_COVIS_MAX_KF, conn_cap <= PGORB_COVIS_MAX_CONN, cap_per_frame <= 16000.  Scratch arena
 * (KeyFrameCulling): (nframes + npoints + 2 * conn_cap) * 4 bytes.  Determinism: a result depends on its inputs alone. */
#define PGORB_CULL_MP_KEEP         0
#define PGORB_CULL_MP_WAS_BAD      1
#define PGORB_CULL_MP_FOUND_RATIO  2
#define PGORB_CULL_MP_FEW_OBS      3
#define PGORB_CULL_MP_AGED         4
#define PGORB_CULL_MP_NONE         5
#define PGORB_CULL_KF_KEEP         0
#define PGORB_CULL_KF_CULLED       1
#define PGORB_CULL_KF_TO_BE_ERASED 2
#define PGORB_CULL_KF_ID0          3
#define PGORB_CULL_KF_WAS_BAD      4
#define PGORB_CULL_KF_NONE         5
#define PGORB_CULL_ROW_ERASED      1
#define PGORB_CULL_ROW_CLEARED     2
#define PGORB_CULL_ROW_REPARENTED  4
#define PGORB_CULL_LIMIT           32
#define PGORB_CULL_INFO            4
int  pgorb_compact_observations_device(pgorb_ctx* ctx,
        int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
        const uint8_t* d_obs_live, const int32_t* d_ref_obs, int32_t* d_obs_start_out, int32_t* d_obs_frame_out, int32_t* d_obs_idx_out,
        int32_t* d_ref_obs_out, int32_t* d_info /*[1]*/, void* hip_stream);
int  pgorb_map_point_culling(pgorb_ctx* ctx,
        int nkf, int32_t* const* kf_point, const int32_t* n /*[nkf]*/, int npoints, uint8_t* point_bad /*[npoints]*/,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, const int32_t* obs_idx, uint8_t* obs_live,
        const int32_t* first_kf_id, const int32_t* visible, const int32_t* found /*[npoints]*/, int nrecent, const int32_t* recent,
        int cur_kf_id, int th_obs, int32_t* action /*[nrecent]*/, int32_t* recent_out /*[nrecent]*/, int32_t* nrecent_out,
        int32_t* info /*[PGORB_CULL_INFO]*/);
int  pgorb_map_point_culling_device(pgorb_ctx* ctx,
        int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, int npoints, uint8_t* d_point_bad,
        const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs, uint8_t* d_obs_live,
        const int32_t* d_first_kf_id, const int32_t* d_visible, const int32_t* d_found, int nrecent, const int32_t* d_recent,
        int cur_kf_id, int th_obs, int32_t* d_action, int32_t* d_recent_out, int32_t* d_nrecent_out, int32_t* d_info, void* hip_stream);
int  pgorb_keyframe_culling(pgorb_ctx* ctx,
        int nkf, const pgorb_keypoint* const* kps, int32_t* const* kf_point, const int32_t* n /*[nkf]*/,
        int npoints, uint8_t* point_bad, const int32_t* obs_start, const int32_t* obs_frame, const int32_t* obs_idx, uint8_t* obs_live,
        int32_t* ref_obs /*[npoints]*/, const int32_t* kf_order /*[nkf] or NULL*/, const uint8_t* kf_id0 /*[nkf] or NULL*/,
        const uint8_t* kf_not_erase /*[nkf] or NULL*/, uint8_t* kf_bad /*[nkf]*/, uint8_t* kf_to_be_erased /*[nkf] or NULL*/, int cur_kf,
        int conn_cap, int32_t* conn_kf, int32_t* conn_w /*[nkf][conn_cap]*/, int32_t* nconn, int32_t* ord_kf, int32_t* ord_w, int32_t* nord,
        int32_t* parent /*[nkf]*/, int list_cap, int32_t* record /*[list_cap][4]*/, int32_t* row_status /*[nkf]*/,
        int32_t* info /*[PGORB_CULL_INFO]*/);
int  pgorb_keyframe_culling_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame,
        int npoints, uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
        uint8_t* d_obs_live, int32_t* d_ref_obs, const int32_t* d_kf_order, const uint8_t* d_kf_id0, const uint8_t* d_kf_not_erase,
        uint8_t* d_kf_bad, uint8_t* d_kf_to_be_erased, int cur_kf,
        int conn_cap, int32_t* d_conn_kf, int32_t* d_conn_w, int32_t* d_nconn, int32_t* d_ord_kf, int32_t* d_ord_w, int32_t* d_nord,
        int32_t* d_parent, int list_cap, int32_t* d_record, int32_t* d_row_status, int32_t* d_info, void* hip_stream);

/* ---- Map edits: MapPoint::AddObservation, Replace and EraseObservation with their KeyFrame slot writes (csrc/map_edit.hip) ------
 * The writer the resident table lacked: the cullings can shrink the observation lists, this block grows and merges them, from an
 * ORDERED edit list on the device.  The conventions of the covisibility and culling blocks hold: key frames are the nframes frames
 * of one resident batch with their slots d_kf_point [nframes][cap_per_frame] + d_n, d_kf_order [nframes] = the rank of each key
 * frame's address (NULL = index order), the lists are the CSR d_obs_start / d_obs_frame / d_obs_idx masked by d_obs_live, IN THE
 * ORDER std::map<KeyFrame*, size_t> ITERATES, with d_ref_obs = the position of mpRefKF in the unmasked list.
 *
 *   pgorb_apply_map_edits_device   applies d_edits [0 .. nedits) -- d_nedits [1], when not NULL, bounds the list from the device --
 *       WITH THE RESULT OF APPLYING THEM ONE AFTER ANOTHER IN LIST ORDER.  In/out: d_kf_point, d_point_bad, d_visible and d_found
 *       (int32, NULL = not carried: read as 0), d_replaced [npoints] (mpReplaced, -1 = none; NULL = not carried).  Read: the CSR
 *       with nobs as the bound, d_obs_live (NULL = all live; a dead entry, or one that names nothing of the batch, does not exist)
 *       and d_ref_obs (one that names a dead entry names no key frame).  Written: a FRESH CSR d_obs_start_out [npoints + 1] /
 *       d_obs_frame_out / d_obs_idx_out with room for obs_cap_out entries and d_ref_obs_out [npoints]; they must not alias the
 *       inputs (PGORB_E_ARG for the same pointer).  The call is therefore also the compaction: a culling followed by an edit needs
 *       no pgorb_compact_observations_device.  The lists of points that an edit names come out sorted by address rank; the others
 *       keep their input order, which the convention above makes the same.
 *         PGORB_EDIT_NOP       padding: producers write fixed positions, nothing is compacted
 *         PGORB_EDIT_ADD       a = point, b = key frame, c = keypoint.  AddObservation (src/MapPoint.cc:119-130): the list is left
 *             alone if it holds b (PGORB_EDIT_ALREADY), else (b, c) joins it; then KeyFrame::AddMapPoint (src/KeyFrame.cc:313-317)
 *             kf_point[b][c] = a, whatever the list did.  No bad test.
 *         PGORB_EDIT_REPLACE   a = loser, b = survivor: a->Replace(b) (:196-232).  a == b: nothing (PGORB_EDIT_SELF).  Else the
 *             loser's list is taken and cleared, the loser goes bad, replaced[a] = b; for each (kf, idx) of it: the survivor does
 *             not hold kf (tested BY ITS LIST, IsInKeyFrame, not by the slot) -> kf_point[kf][idx] = b and (kf, idx) joins the
 *             survivor, else kf_point[kf][idx] = -1; then found[b] += found[a], visible[b] += visible[a].  No bad test on either
 *             side: a loser that is already bad has an empty list and hands its counters over again, as the reference does.  The
 *             ComputeDistinctiveDescriptors at :231 is NOT run; the survivor is reported in d_touched.
 *         PGORB_EDIT_ERASE     a = point, b = key frame.  KeyFrame::EraseMapPointMatch(MapPoint*) (src/KeyFrame.cc:326-331: the index
 *             comes from the POINT's list) and EraseObservation (:132-158): if the list holds (b, idx): kf_point[b][idx] = -1, the
 *             entry leaves; mpRefKF == b becomes the first entry of what is left -- the reference dereferences begin() of an empty
 *             map there, HERE THE REFERENCE KEY FRAME BECOMES NONE; with two or fewer entries left SetBadFlag (:172-187) runs: bad,
 *             the slot of every remaining entry = -1 whatever it holds, the list cleared, mpRefKF kept (PGORB_EDIT_WENT_BAD).  A
 *             point that does not list b is untouched (PGORB_EDIT_NOT_OBSERVED), so later erasures of a point that went bad do nothing.
 *         PGORB_EDIT_SET_REF   a = point, b = key frame: mpRefKF = b (the MapPoint constructor, :47).
 *       The reference key frame is tracked BY KEY FRAME: d_ref_obs_out[p] = its position in the new list, -1 when that list does
 *       not hold it (always for an empty list).  A point or key frame out of range, a keypoint outside [0, d_n[kf]) or an unknown
 *       op makes the edit a no-op with PGORB_EDIT_BAD_INDEX; nothing is read or written out of bounds.
 *       d_edit_status [nedits]: PGORB_EDIT_APPLIED (carried out: ADD also when ALREADY) | ALREADY | SELF | NOT_OBSERVED | WENT_BAD |
 *       BAD_INDEX; 0 for NOP and past d_nedits.  d_touched [npoints]: PGORB_EDIT_TOUCH_CHANGED (the list changed), TOUCH_SURVIVOR
 *       (survivor of a REPLACE: a descriptor is due), TOUCH_STALE (an ADD or ERASE changed the list after the point's last REPLACE
 *       as survivor: the reference's descriptor would be older than its list; counted, not hidden).  d_select_out [sel_cap] (sel_cap
 *       0 = none): the points with d_touched & select_bits, ascending, padded with -1 -- pgorb_refresh_map_points_batch_device
 *       takes -1 as a no-op, so nsel = sel_cap chains without a download.  d_info [PGORB_EDIT_INFO] = (0, the new list length,
 *       edits with APPLIED, points whose bad flag rose, components, slot writes the reference makes, points with TOUCH_STALE, points
 *       selected).  PGORB_EDIT_LIMIT in d_info[0] AND NOTHING ELSE WRITTEN, no in/out byte either: the new lists exceed
 *       obs_cap_out, the selection exceeds sel_cap, a component's live input entries plus its ADD edits exceed
 *       PGORB_EDIT_MAX_BAG, or more than PGORB_EDIT_MAX_EDITS edits are carried out.  The plan finishes in scratch before the first in/out byte changes.
 *       How: no edit reads a slot, so the points linked by REPLACE edits form components that share no state and run independently
 *       (k_edit_components, k_edit_bucket: one workgroup each); k_edit_plan, a wave per component, walks its edits in order over
 *       one bag of (point, key frame, keypoint) in LDS (2 x 24 KiB of the CU's 160 KiB: three waves per CU); a slot takes the value
 *       of the LAST EDIT IN LIST ORDER that writes it, within a component in the bag, across components by an atomicMax of the edit
 *       index whose result no order of execution changes (k_edit_mark, k_edit_commit).  Integers only.  Does not synchronise the stream.
 *   pgorb_apply_map_edits   the same from host buffers (kf_point[f] [n[f]]), checked: returns the number of edits applied (0 with
 *       PGORB_EDIT_LIMIT), or PGORB_E_ARG for a negative count, a NULL array that is read or written, obs_start not rising from 0, a
 *       live observation out of range, a key frame twice in one list, kf_order not a permutation, ref_obs outside its list, an
 *       output overlapping an input, an unknown op; PGORB_E_LIMIT for more than PGORB_EDIT_MAX_EDITS edits that are not NOP.  Byte for byte the device form; output bytes it does not write keep their values.
 *
 * Limits.  PGORB_EDIT_MAX_EDITS bounds the edits that are CARRIED OUT (not NOP, indices in range: the bucket sorts them in LDS), not
 * the length of the list: producers write fixed positions, so a list is as long as its producer's array (cap_per_frame, 2 * qcap,
 * nobs) and mostly NOP.  The device form cannot know the count before it runs: more than PGORB_EDIT_MAX_EDITS such edits give
 * PGORB_EDIT_LIMIT in d_info[0] and nothing else written, like the other capacities; the host form counts the edits that are not NOP
 * and returns PGORB_E_LIMIT.  PGORB_E_LIMIT also for nedits > PGORB_EDIT_MAX_LIST, nframes > PGORB_COVIS_MAX_KF, cap_per_frame > 16000,
 * npoints > 2^30.  THE SLOTS MUST HOLD -1 OR VALUES BELOW 2^30: k_edit_mark keeps its marks (2^30 | edit index) in the slots themselves
 * between two launches, and a slot that already holds a larger value keeps it.  Cost that does not depend on the edits: k_edit_init
 * and k_edit_commit are a thread per point, and k_edit_scan is ONE workgroup of 256 threads that walks all npoints (the lengths, the
 * selection, the counts); with npoints = point_cap of 10^5 that is some 400 points a thread on every call, however short the list.  It
 * has not been measured against a multi-block scan.  Scratch arena: 64 + 40 * npoints + 4 * (nedits + 1) + 8 * (m + 1) + 20 * (nobs + m)
 * bytes with m = min(nedits, PGORB_EDIT_MAX_EDITS), each array rounded up to 64.  Determinism: a result depends on its inputs alone --
 * not on the stream, a repeat, or NOP padding in the list. */
typedef struct pgorb_map_edit { int32_t op, a, b, c; } pgorb_map_edit;
#define PGORB_EDIT_NOP            0
#define PGORB_EDIT_ADD            1
#define PGORB_EDIT_REPLACE        2
#define PGORB_EDIT_ERASE          3
#define PGORB_EDIT_SET_REF        4
#define PGORB_EDIT_APPLIED        1
#define PGORB_EDIT_ALREADY        2
#define PGORB_EDIT_SELF           4
#define PGORB_EDIT_NOT_OBSERVED   8
#define PGORB_EDIT_WENT_BAD       16
#define PGORB_EDIT_BAD_INDEX      32
#define PGORB_EDIT_LIMIT          64
#define PGORB_EDIT_TOUCH_CHANGED  1
#define PGORB_EDIT_TOUCH_SURVIVOR 2
#define PGORB_EDIT_TOUCH_STALE    4
#define PGORB_EDIT_INFO           8
#define PGORB_EDIT_MAX_BAG        2048
#define PGORB_EDIT_MAX_EDITS      4096
#define PGORB_EDIT_MAX_LIST       4194304
int  pgorb_apply_map_edits(pgorb_ctx* ctx,
        const pgorb_map_edit* edits, int nedits, int nkf, int32_t* const* kf_point, const int32_t* n /*[nkf]*/,
        const int32_t* kf_order /*[nkf] or NULL*/, int npoints, uint8_t* point_bad, int32_t* visible, int32_t* found, int32_t* replaced,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, const int32_t* obs_idx, const uint8_t* obs_live /*or NULL*/,
        const int32_t* ref_obs /*[npoints]*/, int obs_cap_out, int32_t* obs_start_out, int32_t* obs_frame_out, int32_t* obs_idx_out,
        int32_t* ref_obs_out, int32_t* edit_status /*[nedits]*/, int32_t* touched /*[npoints]*/, int select_bits, int sel_cap,
        int32_t* select_out /*[sel_cap]*/, int32_t* info /*[PGORB_EDIT_INFO]*/);
int  pgorb_apply_map_edits_device(pgorb_ctx* ctx,
        const pgorb_map_edit* d_edits, int nedits, const int32_t* d_nedits /*[1] or NULL*/, int32_t* d_kf_point, const int32_t* d_n,
        int nframes, int cap_per_frame, const int32_t* d_kf_order, int npoints, uint8_t* d_point_bad, int32_t* d_visible, int32_t* d_found,
        int32_t* d_replaced, const int32_t* d_obs_start, const int32_t* d_obs_frame, const int32_t* d_obs_idx, int nobs,
        const uint8_t* d_obs_live, const int32_t* d_ref_obs, int obs_cap_out, int32_t* d_obs_start_out, int32_t* d_obs_frame_out,
        int32_t* d_obs_idx_out, int32_t* d_ref_obs_out, int32_t* d_edit_status, int32_t* d_touched, int select_bits, int sel_cap,
        int32_t* d_select_out, int32_t* d_info /*[PGORB_EDIT_INFO]*/, void* hip_stream);
/* The producers: each turns one step's device output into edits AT FIXED POSITIONS, PGORB_EDIT_NOP where nothing happens, so the
 * list order is the reference's loop order and nothing is downloaded between the step and pgorb_apply_map_edits_device.  They do
 * not check their inputs beyond NULL and the counts: an index out of range becomes a NOP or an edit that the executor refuses with
 * PGORB_EDIT_BAD_INDEX.  Asynchronous on hip_stream, no scratch.  The tail of CreateNewMapPoints (src/LocalMapping.cc:436-449) has no
 * producer: appending its rows to the table and writing SET_REF(new, kf1), ADD(new, kf1, idx1), ADD(new, kf2, idx2) per record is the caller's.
 *   pgorb_map_edits_from_keyframe_device   LocalMapping::ProcessNewKeyFrame's loop (src/LocalMapping.cc:142-161) for key frame kf:
 *       d_edits [cap_per_frame], d_slot_class [cap_per_frame].  Slot i holding an in-range, not-bad point P: P does not list kf
 *       (live entries only) and no lower slot of kf holds P -> ADD(P, kf, i) at edit i, class 1; else NOP, class 2 (the else branch
 *       of :155: mlpRecentAddedMapPoints.push_back) -- a lower slot's ADD makes IsInKeyFrame true.  Every other slot: NOP, class
 *       0.  UpdateNormalAndDepth / ComputeDistinctiveDescriptors of the class-1 points is the refresh that follows the apply.  A
 *       thread per slot; it looks through the lower slots itself.
 *   pgorb_map_edits_from_fuse_device   ONE problem of pgorb_fuse_batch_device (src/ORBmatcher.cc:961-979): d_nq [1], d_queries,
 *       d_action, d_best_idx [qcap] are that problem's rows, kf its key frame.  d_replace_point == NULL, d_edits [qcap]: ADDED ->
 *       ADD(query, kf, best_idx); MERGED_INTO_KF_POINT -> REPLACE(query, occupant); REPLACED_KF_POINT -> REPLACE(occupant, query),
 *       the occupant being the slot's RUNNING occupant: its entry value, or the latest earlier query with the same best_idx and
 *       action ADDED or REPLACED_KF_POINT.  With d_replace_point (one problem of pgorb_fuse_sim3_batch_device,
 *       src/LoopClosing.cc:601-615), d_edits [2 * qcap]: the ADDs at [0, qcap) and REPLACE(replace_point[q], query) at [qcap,
 *       2 qcap): Fuse runs to its end before the replacements.
 *   pgorb_map_edits_from_lba_erase_device   src/Optimizer.cc:748-757 for one window of pgorb_local_bundle_adjustment_batch_device:
 *       CSR position j with d_erase[j] set -> ERASE(the point of j, obs_frame[j]) at edit j of d_edits [nobs].  A point's erasures
 *       stay in list order, the order of the reference's edges.
 *   pgorb_map_edits_from_loop_matches_device   src/LoopClosing.cc:520-537: d_matched [cap_per_frame] = mvpCurrentMatchedPoints as
 *       table indices (-1 = NULL) for cur_kf; a slot with an occupant -> REPLACE(occupant, matched), an empty one -> ADD(matched,
 *       cur_kf, i), at edit i of d_edits [cap_per_frame].  Taken from the entry state, which is exact: an occupant lists cur_kf
 *       only at its own slot, so no earlier edit of the loop writes slot i.
 *   pgorb_observation_ids_device   d_obs_kf_out[o] = d_kf_id[obs_frame[o]], each list sorted ascending: the obs_kf CSR that
 *       pgorb_fuse_batch_device reads, so that edit -> refresh -> the next target's Fuse chains without a download. */
int  pgorb_map_edits_from_keyframe_device(pgorb_ctx* ctx,
        const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, int npoints, const uint8_t* d_point_bad,
        const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint8_t* d_obs_live /*or NULL*/, int kf,
        pgorb_map_edit* d_edits, int32_t* d_slot_class, void* hip_stream);
int  pgorb_map_edits_from_fuse_device(pgorb_ctx* ctx,
        const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, int npoints, int kf, int qcap,
        const int32_t* d_nq, const int32_t* d_queries, const int32_t* d_action, const int32_t* d_best_idx,
        const int32_t* d_replace_point /*or NULL*/, pgorb_map_edit* d_edits, void* hip_stream);
int  pgorb_map_edits_from_lba_erase_device(pgorb_ctx* ctx,
        int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint8_t* d_erase, pgorb_map_edit* d_edits,
        void* hip_stream);
int  pgorb_map_edits_from_loop_matches_device(pgorb_ctx* ctx,
        const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, int npoints, int cur_kf,
        const int32_t* d_matched, pgorb_map_edit* d_edits, void* hip_stream);
int  pgorb_observation_ids_device(pgorb_ctx* ctx,
        int npoints, const int32_t* d_obs_start, const int32_t* d_obs_frame, int nobs, const uint64_t* d_kf_id, int nframes,
        uint64_t* d_obs_kf_out, void* hip_stream);

/* ---- Loop correction: CorrectLoop's propagation and the map update after global bundle adjustment (csrc/loop_correct.hip) ------
 * The two map rewrites between loop closing's numerical steps, on the arrays those steps read and write, so that ComputeSim3 ->
 * correction -> Fuse(Sim3) -> UpdateConnections -> OptimizeEssentialGraph -> GlobalBundleAdjustment -> map update -> refresh is one
 * stream of launches.  The conventions of the covisibility block hold: key frames are the nframes frames of one resident batch with
 * their slots d_kf_point [nframes][cap_per_frame] + d_n, the table is that of pgorb_refresh_map_points (d_points, d_point_bad (NULL
 * = none), the CSR d_obs_start / d_obs_frame / d_obs_idx, d_ref_obs), d_kf_order is the address rank (NULL = index order), an index
 * out of range is no slot, no observation and no key frame, and the device forms never read or write out of bounds.  The library is
 * built with -ffp-contract=off and these paths use + - x / and correctly rounded square roots only: every result is exact.
 *
 *   pgorb_correct_loop_poses_device   LoopClosing::CorrectLoop, :438-516, without the per-member UpdateConnections() of :515 (that
 *       is pgorb_update_connections_batch_device with the members in address order) and without the Replace bookkeeping of :520-537.
 *       Inputs: d_kps (only `octave` is read), d_pose (Tcw and Ow are read AS GIVEN; the camera is copied through), cur_kf, d_scw =
 *       mg2oScw (one pgorb_sim3d on the device, e.g. where OptimizeSim3 left it), d_list [nlist] = mvpCurrentConnectedKFs: an entry
 *       that is negative, out of range or cur_kf is skipped, one named twice counts once, and the library adds cur_kf itself.  A
 *       row of d_ord_kf may therefore be passed with its whole capacity (d_list = d_ord_kf + cur_kf * conn_cap, nlist = conn_cap),
 *       BUT WITH ITS COUNT: past a row's count the padding is not reliably -1.  The cullings write -1 into the entries a row
 *       loses, but pgorb_update_connections_batch_device writes entries [0, nord) only, so a row that it made shorter keeps stale
 *       key-frame indices behind its count (and a row it never wrote holds whatever the caller put there; pilotguru_amd's
 *       CovisibilityGraph starts with -1).  d_list_count (NULL = nlist) is that count on the device, d_nord + cur_kf: entries at
 *       or past min(nlist, *d_list_count) are not read as members.  d_ref_kf [npoints] = GetReferenceKeyFrame() by index, -1 = none.
 *       Members = the list + cur_kf.  NonCorrectedSim3[i] = Sim3(Quaterniond(Riw), tiw, 1); CorrectedSim3[cur] = scw byte for byte;
 *       for the others Sim3(Ric, tic, 1) * scw with Tic = Tiw * Twc, a 4 x 4 float product, Twc = [Rcw' | Ow]
 *       of cur_kf.  The point loop runs over CorrectedSim3, a std::map<KeyFrame*, ..>: a live point is corrected ONCE, by the member
 *       of smallest address rank that holds it in a slot (mnCorrectedByKF): pos = correctedSwi.map(Siw.map(pos)) in double, rounded
 *       to float.  Then UpdateNormalAndDepth in the state the reference is in at that moment: with i the correcting member, an
 *       observing key frame j contributes its CORRECTED camera centre if and only if j is a member and rank(j) < rank(i) strictly
 *       (i's own SetPose follows its point loop, :512), every other observer the centre passed in; the reference key frame (the
 *       observation d_ref_obs names) by the same rule.  In a consistent map (every observing member holds the point in a slot) all
 *       centres are the ones passed in.  A list longer than PGORB_MP_MAX_OBS: the position is corrected, normal and distances keep
 *       their bytes, PGORB_LC_OVER_OBS.  An empty list: the same, silently (MapPoint.cc:362-363).  In the device form a list outside
 *       [0, nobs], an observation outside the batch or a d_ref_obs outside its list does the same with PGORB_LC_BAD_INDEX.
 *       Outputs, exactly what pgorb_optimize_essential_graph_device reads: d_has_corrected / d_corrected / d_has_non_corrected /
 *       d_non_corrected [nframes] (flag 0 and a zero record for a key frame that is no member); d_pose_out [nframes] (must not be
 *       d_pose): for members [R | t/s] through Converter::toCvSE3 to float, then SetPose's Ow, the camera kept; the input's bytes
 *       for the others; the table in place (pos, normal, min_distance, max_distance of the corrected points); d_corrected_by
 *       [npoints] = the correcting key frame or -1 (mnCorrectedReference); d_point_ref_kf [npoints] = d_corrected_by where it is
 *       set, else d_ref_kf -- the array the essential graph takes; d_info [PGORB_LC_INFO] = status bits, members, points corrected,
 *       points over the observation limit.  Launches: k_lc_init, k_lc_rank (with a d_kf_order), k_lc_members (a thread per member),
 *       k_lc_claim (a thread per (member, slot): an integer atomicMin of the address rank per point -- a minimum has no order),
 *       k_lc_points (a thread per point); no floating-point atomic, no host round trip.  Scratch arena: (2 nframes + npoints) * 4.
 *   pgorb_global_ba_map_update_device   LoopClosing::RunGlobalBundleAdjustment, :679-742.  d_pose = the poses as local mapping left
 *       them (what becomes mTcwBefGBA); d_pose_gba / d_kf_done / d_pos_gba / d_point_done as pgorb_global_bundle_adjustment_device
 *       writes them; d_parent the covisibility graph's; d_kf_origin [nframes] (uint8) = is in mvpKeyFrameOrigins; d_kf_bad (NULL =
 *       none); d_ref_kf as above.  A key frame is VISITED when it is not bad and its parent chain reaches an origin without passing
 *       a bad key frame or a cycle (the chain ends at the first origin; an origin's own parent is not followed).  A visited key
 *       frame that is done takes d_pose_gba's record.  A visited one that is not done takes (Tcw_child * Twc_parent) *
 *       TcwGBA_parent: two 4 x 4 float products, Twc_parent = [Rcw' | Ow] of the parent's pose BEFORE the update, TcwGBA_parent the
 *       parent's result; then SetPose's Ow, the camera kept.  Both operands of the first product are pre-update poses, so the result
 *       depends on the chain down from the nearest done ancestor alone and is multiplied in exactly that order -- float rounding
 *       forbids regrouping.  ONE DEPARTURE: a key frame that is not visited, or whose chain holds no done key frame up to its origin
 *       (the reference would read a stale mTcwGBA there), keeps its input bytes and gets d_kf_updated = 0.  Cost: a thread per key
 *       frame walks up its chain (depth d) and multiplies down it, finding each ancestor by walking again: d products and d^2 / 2
 *       parent reads per key frame, so a tree of depth d costs at most nframes * d^2 / 2 reads (13.5 M for a chain of 300); no cap
 *       on the depth other than nframes, and two launches (k_mu_kf, k_mu_points) whatever the tree's depth.
 *       Points: a bad point keeps its bytes; a done point takes d_pos_gba; otherwise, when d_ref_kf is valid and that key frame
 *       was updated, pos = Rwc_new * (Rcw_bef * pos + tcw_bef) + Ow_new on gemm's small-matrix path with the translation folded
 *       into C (kf_row); any other point keeps its bytes.  No UpdateNormalAndDepth follows in the reference;
 *       pgorb_refresh_map_points_batch_device with PGORB_MP_NORMAL_DEPTH may be chained.  Outputs:
 *       d_pose_out (must not be d_pose), d_kf_updated [nframes], d_points[].pos in place, d_point_updated [npoints], d_info
 *       [PGORB_MU_INFO] = 0, key frames updated, of those recomputed, points updated.
 *   pgorb_correct_loop_poses / pgorb_global_ba_map_update   the same from host buffers (kps[f], kf_point[f] [n[f]]; scw on the
 *       host), checked on the host before anything else: PGORB_E_ARG for a negative count, a NULL array that is read or written,
 *       cur_kf, a slot, an observation (key frame or keypoint), ref_kf or a parent out of range, kf_order not a permutation, a pose
 *       (Tcw, Ow), scw, a point or a done result that is not finite, a scale <= 0, obs_start not rising from 0, ref_obs outside the
 *       list of a live point with 1 .. PGORB_MP_MAX_OBS observations, a key frame twice in one list, a parent cycle.  They return the number of points corrected /
 *       key frames updated and equal the device forms byte for byte.  The device forms check pointers and limits only.
 * Limits (PGORB_E_LIMIT): nframes and nlist <= PGORB_COVIS_MAX_KF, cap_per_frame <= 16000.  Determinism: a result depends on its
 * inputs alone, not on the stream, a repeat or what the context ran before. */
#define PGORB_LC_OVER_OBS  1
#define PGORB_LC_BAD_INDEX 2
#define PGORB_LC_INFO      4
#define PGORB_MU_INFO      4
int  pgorb_correct_loop_poses(pgorb_ctx* ctx,
        int nkf, const pgorb_keypoint* const* kps, const int32_t* n /*[nkf]*/, const pgorb_kf_pose* pose /*[nkf]*/, int cur_kf,
        const pgorb_sim3d* scw, int nlist, const int32_t* list, const int32_t* kf_order /*[nkf] or NULL*/,
        const int32_t* const* kf_point /*[nkf][n[f]]*/, int npoints, pgorb_map_point* points /*in and out*/,
        const uint8_t* point_bad /*[npoints] or NULL*/, const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame,
        const int32_t* obs_idx, const int32_t* ref_obs /*[npoints]*/, const int32_t* ref_kf /*[npoints]*/,
        uint8_t* has_corrected, pgorb_sim3d* corrected, uint8_t* has_non_corrected, pgorb_sim3d* non_corrected /*[nkf]*/,
        pgorb_kf_pose* pose_out /*[nkf]*/, int32_t* corrected_by, int32_t* point_ref_kf /*[npoints]*/, int32_t* info /*[PGORB_LC_INFO]*/);
int  pgorb_correct_loop_poses_device(pgorb_ctx* ctx,
        const pgorb_keypoint* d_kps, const int32_t* d_n, int nframes, int cap_per_frame, const pgorb_kf_pose* d_pose, int cur_kf,
        const pgorb_sim3d* d_scw, int nlist, const int32_t* d_list, const int32_t* d_list_count /*[1] or NULL*/,
        const int32_t* d_kf_order, const int32_t* d_kf_point, int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        const int32_t* d_obs_idx, int nobs, const int32_t* d_ref_obs, const int32_t* d_ref_kf,
        uint8_t* d_has_corrected, pgorb_sim3d* d_corrected, uint8_t* d_has_non_corrected, pgorb_sim3d* d_non_corrected,
        pgorb_kf_pose* d_pose_out, int32_t* d_corrected_by, int32_t* d_point_ref_kf, int32_t* d_info, void* hip_stream);
int  pgorb_global_ba_map_update(pgorb_ctx* ctx,
        int nkf, const pgorb_kf_pose* pose, const pgorb_kf_pose* pose_gba /*[nkf]*/, const uint8_t* kf_done /*[nkf]*/,
        const int32_t* parent /*[nkf]*/, const uint8_t* kf_origin /*[nkf]*/, const uint8_t* kf_bad /*[nkf] or NULL*/,
        int npoints, pgorb_map_point* points /*in and out: pos*/, const float* pos_gba /*[npoints][3]*/, const uint8_t* point_done,
        const uint8_t* point_bad /*[npoints] or NULL*/, const int32_t* ref_kf /*[npoints]*/,
        pgorb_kf_pose* pose_out /*[nkf]*/, uint8_t* kf_updated /*[nkf]*/, uint8_t* point_updated /*[npoints]*/, int32_t* info /*[PGORB_MU_INFO]*/);
int  pgorb_global_ba_map_update_device(pgorb_ctx* ctx,
        int nframes, const pgorb_kf_pose* d_pose, const pgorb_kf_pose* d_pose_gba, const uint8_t* d_kf_done, const int32_t* d_parent,
        const uint8_t* d_kf_origin, const uint8_t* d_kf_bad,
        int npoints, pgorb_map_point* d_points, const float* d_pos_gba, const uint8_t* d_point_done, const uint8_t* d_point_bad,
        const int32_t* d_ref_kf, pgorb_kf_pose* d_pose_out, uint8_t* d_kf_updated, uint8_t* d_point_updated, int32_t* d_info,
        void* hip_stream);

/* ---- The trajectory read-out: Tracking's pose record and System::GetTrajectory (csrc/track_pose.hip) ---------------------------
 * The pose bookkeeping at the head and the tail of Tracking::Track and the function that turns it into the trajectory, on resident
 * arrays, so that predict -> SearchByProjection(last frame) -> PoseOptimization -> UpdateLocalMap -> SearchLocalPoints ->
 * PoseOptimization -> commit runs frame after frame without a pose leaving the device, and the finished ride is read out in the
 * layout pgorb_smooth_heading_directions / pgorb_trajectory_pca / pgorb_project_directions take.  Restates (thirdparty/orb-slam2):
 *   Tracking::UpdateLastFrame (monocular return)     src/Tracking.cc:792-798      Tlr * pRef->GetPose()
 *   TrackWithMotionModel / TrackReferenceKeyFrame    :866 / :764                   mVelocity * mLastFrame.mTcw / mLastFrame.mTcw
 *   Tracking::Track, the motion model and the record :432-440, :493, :497-506     mTcw * LastTwc, mTcw * refKF->GetPoseInverse()
 *   KeyFrame::SetBadFlag's mTcp                      src/KeyFrame.cc:641          Tcw * mpParent->GetPoseInverse()
 *   System::GetTrajectory                            src/System.cc:371-412
 * Every product is the 4 x 4 float product of DESIGN.md section 4 (gemm's small-matrix path, four terms in index order, the fourth
 * formed), every SetPose gives Ow = -Rcw.t()*tcw with alpha = -1 applied in double, GetPoseInverse() is [Rcw' | Ow] of the pose AS
 * GIVEN.  The library is built with -ffp-contract=off and these paths use + - x and correctly rounded square roots and divisions
 * only: every result is exact.  The key-frame table is what the other calls take: d_pose (Tcw and Ow are read), d_kf_bad, d_parent,
 * d_kf_id (mnId) over nkf key frames -- several rides share one table and name their key frames by table index -- plus d_tcp
 * [nkf][12] = mTcp rows 0-2, meaningful only where kf_bad is set.
 *
 *   pgorb_track_state         one tracker's pose members: `last` = mLastFrame as a complete pgorb_kf_pose (has_last =
 *       !mLastFrame.mTcw.empty()), velocity = mVelocity rows 0-2 (has_velocity), last_ref_kf = mLastFrame.mpReferenceKF.
 *   pgorb_trajectory_record   RelativeFramePoseData (include/Tracking.h:58-64): pose = mRelativeFramePose rows 0-2 (has_pose),
 *       ref_kf = mpReference, frame_time = mFrameTime, frame_id = mFrameId, lost = mbLost.
 *   A tracker's records are d_traj + t * traj_cap, d_ntrajectory[t] of them (mlTrajectory).
 *
 *   pgorb_track_predict_batch_device   the pose the first search of a frame starts from, a thread per tracker.  d_mode [ntrack]
 *       (NULL = `mode` for all).  PGORB_TRACK_MOTION_MODEL: UpdateLastFrame -- state.last takes Tcw = record.pose *
 *       Tcw[last_ref_kf] of the tracker's LAST record, then SetPose's Ow, written back to the state -- then pose_out = velocity *
 *       last.Tcw with SetPose's Ow.  PGORB_TRACK_REFERENCE_KF: pose_out = state.last as it stands, no UpdateLastFrame.
 *       d_pose_out [ntrack] are complete records with the camera of state.last, what
 *       pgorb_search_by_projection_last_frame_batch_device and pgorb_pose_optimization_batch_device take as d_pose.  d_status
 *       [ntrack]: 0, or PGORB_TRACK_NO_LAST (has_last == 0), PGORB_TRACK_NO_VELOCITY (motion model with has_velocity == 0),
 *       PGORB_TRACK_BAD_INDEX (motion model: last_ref_kf outside [0, nkf), no record, a count past traj_cap or a last record
 *       without a pose; any mode: a mode that is neither); with a status the state is not written and pose_out is state.last
 *       unchanged.
 *   pgorb_track_commit_batch_device   the end of Track(), a thread per tracker, in the reference's order.  Inputs per tracker:
 *       d_pose = the frame's final pose (as PoseOptimization wrote it), d_ok = bOK, d_ref_kf = mpReferenceKF after a possible
 *       CreateNewKeyFrame, d_frame_time, d_frame_id.  (1) with bOK: velocity = pose.Tcw * [Rlast' | Ow_last] when has_last, else
 *       has_velocity = 0; without bOK the velocity is LEFT AS IT IS (the reference does not clear it on a lost frame); (2) the
 *       record (pose.Tcw * GetPoseInverse() of ref_kf, ref_kf, time, id, lost = !bOK, has_pose = 1) is appended at
 *       d_ntrajectory[t] and the count advances; (3) state.last = pose, has_last = 1, last_ref_kf = ref_kf.  d_status: 0,
 *       PGORB_TRACK_FULL (the count is outside [0, traj_cap)) or PGORB_TRACK_BAD_INDEX (ref_kf outside [0, nkf)); with a status
 *       NOTHING is written, neither state, record nor count.
 *   pgorb_keyframe_tcp_device   mTcp of every record of a pgorb_keyframe_culling_device call whose action is
 *       PGORB_CULL_KF_CULLED: reads d_record [list_cap][4] and d_cull_info (that call's d_info: nothing is done with
 *       PGORB_CULL_LIMIT, else min(d_cull_info[1], list_cap) records are looked at) where that call left them, d_pose and d_parent;
 *       writes d_tcp[A] = Tcw[A] * GetPoseInverse(parent[A]) for the culled A only, every other row keeps its bytes.  A key
 *       frame outside [0, nframes) or a parent outside it (-1 = none) leaves the row untouched and counts.  d_info_out
 *       [PGORB_TCP_INFO] = (0, rows written, rows skipped).  IT MUST RUN AFTER THE CULLING AND BEFORE THE NEXT CALL THAT MOVES A
 *       POSE (local bundle adjustment, loop correction, the map update after global bundle adjustment): mTcp is the relative pose
 *       frozen at the moment of the cull, and the culling keeps parent[A] for exactly this.  A thread per record.
 *   pgorb_get_trajectory_device   System::GetTrajectory over the first min(n, *d_count) records of d_traj (d_count NULL = n;
 *       d_ntrajectory + t of a tracker), to be launched once per tracker.  k_traj_origin (one workgroup) finds Two =
 *       GetPoseInverse() of the key frame with the smallest d_kf_id among kf_bad == 0 (the smaller index on equal ids) --
 *       Map::GetAllKeyFrames sorted by lId, from which erased key frames are gone -- and leaves its index in d_info[1]; no live key
 *       frame: d_info[0] = PGORB_TRAJ_NO_ORIGIN and no output is written.  k_traj_records, a thread per record: time_usec =
 *       (int64)(frame_time * 1e6), one double product truncated toward zero (NaN or outside int64: INT64_MIN, what x86-64's
 *       cvttsd2si returns, and PGORB_TRAJ_BAD_TIME), frame_id, is_lost; a lost record gives seven zeros (Pose() is
 *       value-initialised) and its pose is not read.  Otherwise Trw = eye(4); while kf_bad[k]: Trw = Trw * mTcp[k], k = parent[k]
 *       (the product with the identity is formed: it decides the sign of a zero); then Tcw = record.pose * ((Trw * Tcw[k]) * Two);
 *       quat_wxyz = Eigen's Quaterniond of the TRANSPOSED 3 x 3 block widened to double; translation = -R' * t on gemm's
 *       small-matrix path with alpha = -1 in double, rounded to float, widened.  The walk is bounded by nkf steps:
 *       a parent of -1 under a bad key frame, an index outside [0, nkf), a cycle of bad key frames, or has_pose == 0 on a record
 *       that is not lost gives PGORB_TRAJ_BROKEN in d_status[i] and seven zeros, the other records unaffected.  Outputs
 *       d_quat_wxyz [n][4], d_translation [n][3] (double), d_time_usec, d_frame_id [n] (int64), d_is_lost [n] (uint8), d_status
 *       [n]; entries at or past the count keep their bytes.  d_info [PGORB_TRAJ_INFO] = (status, origin key frame or -1, broken
 *       records, records).
 *   pgorb_track_predict / pgorb_track_commit / pgorb_keyframe_tcp / pgorb_get_trajectory   the same from host buffers, checked on
 *       the host before anything else, byte for byte equal to the device forms.  predict and commit take ONE tracker (its state
 *       in/out, for predict its last record or NULL, for commit its record array and count in/out) and return its status;
 *       keyframe_tcp takes nrecord records and returns the rows written; get_trajectory returns the number of records that are
 *       neither lost nor broken.  PGORB_E_ARG: a negative count, a NULL array that is read or written, an unknown mode; and for
 *       pgorb_get_trajectory also: no live key frame, a record that is not lost with ref_kf outside [0, nkf), a bad key frame whose
 *       parent is -1 or out of range, a frame_time that is not finite or whose product with 1e6 lies outside int64.
 * bOK, the nmatches retry, NeedNewKeyFrame / CreateNewKeyFrame and CheckReplacedInLastFrame are the block below (csrc/track_decide.hip).
 * Left to the caller: the relocalisation bookkeeping (mnLastRelocFrameId), System::Reset, and the stereo / RGB-D and mbOnlyTracking
 * branches of UpdateLastFrame.
 * Limits (PGORB_E_LIMIT): nkf <= PGORB_COVIS_MAX_KF, n and traj_cap <= PGORB_TRAJ_MAX_RECORDS, ntrack <= PGORB_TRACK_MAX, list_cap
 * <= PGORB_COVIS_MAX_KF.  No scratch arena: the origin reduction's result lives in d_info.  Determinism: a result depends on its
 * inputs alone, not on the batch size, the stream or a repeat. */
#define PGORB_TRACK_MOTION_MODEL  0
#define PGORB_TRACK_REFERENCE_KF  1
#define PGORB_TRACK_NO_LAST       1
#define PGORB_TRACK_NO_VELOCITY   2
#define PGORB_TRACK_BAD_INDEX     4
#define PGORB_TRACK_FULL          8
#define PGORB_TRACK_MAX           4096
#define PGORB_TRAJ_BROKEN         1
#define PGORB_TRAJ_BAD_TIME       2
#define PGORB_TRAJ_NO_ORIGIN      4
#define PGORB_TRAJ_INFO           4
#define PGORB_TRAJ_MAX_RECORDS    (1 << 22)
#define PGORB_TCP_INFO            4
typedef struct pgorb_track_state {
    pgorb_kf_pose last;      /* mLastFrame: mTcw rows 0-2, mOw, the camera */
    float velocity[12];      /* mVelocity rows 0-2 */
    int32_t last_ref_kf;     /* mLastFrame.mpReferenceKF */
    uint8_t has_last, has_velocity, pad[2];
} pgorb_track_state;
typedef struct pgorb_trajectory_record {
    float pose[12];          /* mRelativeFramePose rows 0-2 */
    int32_t ref_kf;          /* mpReference */
    uint8_t has_pose, lost, pad[2];
    double frame_time;       /* mFrameTime */
    int64_t frame_id;        /* mFrameId */
} pgorb_trajectory_record;
int  pgorb_track_predict(pgorb_ctx* ctx,
        int mode, pgorb_track_state* state /*in and out*/, const pgorb_trajectory_record* last_record /*or NULL*/,
        int nkf, const pgorb_kf_pose* kf_pose /*[nkf]*/, pgorb_kf_pose* pose_out);
int  pgorb_track_predict_batch_device(pgorb_ctx* ctx,
        int ntrack, int mode, const int32_t* d_mode /*[ntrack] or NULL*/, pgorb_track_state* d_state,
        const pgorb_trajectory_record* d_traj /*[ntrack][traj_cap]*/, int traj_cap, const int32_t* d_ntrajectory /*[ntrack]*/,
        int nkf, const pgorb_kf_pose* d_kf_pose, pgorb_kf_pose* d_pose_out /*[ntrack]*/, int32_t* d_status /*[ntrack]*/, void* hip_stream);
int  pgorb_track_commit(pgorb_ctx* ctx,
        pgorb_track_state* state /*in and out*/, const pgorb_kf_pose* pose, int ok, int ref_kf, double frame_time, int64_t frame_id,
        int nkf, const pgorb_kf_pose* kf_pose /*[nkf]*/, pgorb_trajectory_record* traj /*[traj_cap]*/, int traj_cap,
        int32_t* ntrajectory /*in and out*/);
int  pgorb_track_commit_batch_device(pgorb_ctx* ctx,
        int ntrack, pgorb_track_state* d_state, const pgorb_kf_pose* d_pose /*[ntrack]*/, const uint8_t* d_ok, const int32_t* d_ref_kf,
        const double* d_frame_time, const int64_t* d_frame_id /*[ntrack]*/, int nkf, const pgorb_kf_pose* d_kf_pose,
        pgorb_trajectory_record* d_traj /*[ntrack][traj_cap]*/, int traj_cap, int32_t* d_ntrajectory /*[ntrack]*/,
        int32_t* d_status /*[ntrack]*/, void* hip_stream);
int  pgorb_keyframe_tcp(pgorb_ctx* ctx,
        int nkf, const pgorb_kf_pose* pose /*[nkf]*/, const int32_t* parent /*[nkf]*/, int nrecord, const int32_t* record /*[nrecord][4]*/,
        float* tcp /*[nkf][12] in and out*/, int32_t* info_out /*[PGORB_TCP_INFO]*/);
int  pgorb_keyframe_tcp_device(pgorb_ctx* ctx,
        int nframes, const pgorb_kf_pose* d_pose, const int32_t* d_parent, int list_cap, const int32_t* d_record,
        const int32_t* d_cull_info /*[PGORB_CULL_INFO]*/, float* d_tcp, int32_t* d_info_out, void* hip_stream);
int  pgorb_get_trajectory(pgorb_ctx* ctx,
        int nkf, const pgorb_kf_pose* pose /*[nkf]*/, const uint8_t* kf_bad /*[nkf]*/, const int32_t* parent /*[nkf]*/,
        const uint64_t* kf_id /*[nkf]*/, const float* tcp /*[nkf][12]*/, int n, const pgorb_trajectory_record* traj /*[n]*/,
        double* quat_wxyz /*[n][4]*/, double* translation /*[n][3]*/, int64_t* time_usec, int64_t* frame_id /*[n]*/,
        uint8_t* is_lost /*[n]*/, int32_t* status /*[n]*/, int32_t* info /*[PGORB_TRAJ_INFO]*/);
int  pgorb_get_trajectory_device(pgorb_ctx* ctx,
        int nkf, const pgorb_kf_pose* d_pose, const uint8_t* d_kf_bad, const int32_t* d_parent, const uint64_t* d_kf_id,
        const float* d_tcp, int n, const pgorb_trajectory_record* d_traj, const int32_t* d_count /*[1] or NULL*/,
        double* d_quat_wxyz, double* d_translation, int64_t* d_time_usec, int64_t* d_frame_id, uint8_t* d_is_lost,
        int32_t* d_status, int32_t* d_info /*[PGORB_TRAJ_INFO]*/, void* hip_stream);

/* ---- Tracking's decisions: point statistics, bOK, NeedNewKeyFrame, the scene median depth (csrc/track_decide.hip) ----------------
 * The glue between the tracking thread's numeric steps, on the arrays those steps read and write, so that a monocular,
 * mapping-enabled Tracking::Track() runs from CheckReplacedInLastFrame to the trajectory record without a per-keypoint array
 * leaving the device: check_replaced -> predict -> SearchByProjection(last frame) -> PoseOptimization -> decide ->
 * query_seen_from_outliers -> UpdateLocalMap -> SearchLocalPoints -> increase_visible -> PoseOptimization -> decide(LOCAL_MAP) ->
 * finish -> commit.  Restates (thirdparty/orb-slam2):
 *   Tracking::CheckReplacedInLastFrame                   src/Tracking.cc:735-745
 *   SearchLocalPoints' two IncreaseVisible               :1148, :1168
 *   the discard loops' mnLastFrameSeen                   :781, :904
 *   bOK of TrackReferenceKeyFrame, TrackWithMotionModel, TrackLocalMap    :760, :789; :879-886, :918; :932-964
 *   Track()'s tail                                       :445-476 with NeedNewKeyFrame :968-1052, CreateNewKeyFrame :1054-1132
 *   KeyFrame::TrackedMapPoints, ComputeSceneMedianDepth  src/KeyFrame.cc:353-378, :736-766
 *   CreateInitialMapMonocular's unit median depth        src/Tracking.cc:684-709
 * Only the monocular, !mbOnlyTracking branches; stereo / RGB-D, mbVO and localisation mode are out of scope.
 * Conventions.  "Tracker t" is row t of the [ntrack][cap_per_frame] arrays (slots, outlier flags) and entry t of the [ntrack] arrays,
 * as in pgorb_track_predict_batch_device; its frame is d_frame[t] (NULL = frame t) of the nframes frames of one resident batch and
 * its slot count min(max(d_n[frame], 0), cap_per_frame); a frame out of range has no slots; entries of a row at or past the count
 * are neither read nor written.  The table is that of the map-edit block: d_point_bad (NULL = none), d_visible, d_found, d_replaced,
 * the CSR d_obs_start / d_obs_frame bounded by nobs and masked by d_obs_live (NULL = all live; a dead entry, or one that names nothing
 * of the batch, does not exist), and d_kf_point [nframes][cap_per_frame] + d_n; d_point_has_obs (NULL = all 1) is the array the
 * frame's searches and PoseOptimization took.  The _batch_device / _device forms are asynchronous on hip_stream, do not synchronise
 * it and do not check indices: a table index outside [0, npoints) counts as "no point" and is copied through unchanged; nothing is
 * read or written out of bounds.  d_run [ntrack] (NULL = all run) gates a tracker.
 *
 *   pgorb_check_replaced_batch_device   in place on d_last_point: a slot p with d_replaced[p] >= 0 becomes d_replaced[p].  ONE
 *       step: the reference does not follow chains.  A thread per slot.
 *   pgorb_increase_visible_batch_device   from what pgorb_search_local_points_batch_device wrote: d_visible[p] += 1 for every slot of
 *       d_kp_point (its d_kp_point_out: the slots after the bad ones were cleared) that holds a point, and for every query q <
 *       d_nq[t] with d_in_view set; a point held by two slots of a frame counts twice, as in the reference.  int32 atomicAdd on vector
 *       memory: the result does not depend on the order of execution.
 *   pgorb_query_seen_from_outliers_batch_device   the d_query_seen of pgorb_search_local_points: d_query_seen[t][q] = 1 iff some slot
 *       i of tracker t was DISCARDED and d_kp_point[i] == d_queries[t][q], for q < d_nq[t].  d_kp_point is the first stage's slots
 *       BEFORE the discard (what PoseOptimization was given).  A slot counts as discarded when d_outlier[i] is set (d_outlier NULL =
 *       no flags) or when d_kp_point_opt[i] != d_kp_point[i] (d_kp_point_opt NULL = not compared); one of the two is required.
 *       PoseOptimization with discard_outliers = 1 CLEARS the flags of the slots it empties, so after that run the flags say
 *       nothing and d_kp_point_opt = its d_kp_point_out is the input to pass (d_outlier NULL or its zeros); the flags serve a
 *       discard_outliers = 0 run.  One bit per table point and tracker in scratch: memset, a thread per slot (atomicOr), a thread
 *       per query.
 *   pgorb_track_decide_batch_device   bOK of one stage and what the reference leaves in mCurrentFrame, a workgroup per tracker.  d_mode
 *       [ntrack] (NULL = `mode` for all); PGORB_DECIDE_MOTION_MODEL and PGORB_DECIDE_REFERENCE_KF equal the PGORB_TRACK_ modes, so
 *       predict's d_mode serves.  Inputs: d_nmatches = the count of the search that counts, d_nmatches_map = PoseOptimization's
 *       (discard_outliers = 1), d_pose_opt / d_kp_point_opt = PoseOptimization's d_pose_out / d_kp_point_out, d_pose_before /
 *       d_kp_point_before = what the frame holds when the stage returns early.
 *         PGORB_DECIDE_REFERENCE_KF: nmatches < 15 (int) -> ok = 0, final = before (the frame's entry slots and entry pose, byte
 *             for byte: the reference returns before either is assigned); else ok = nmatches_map >= 10, final = opt.
 *         PGORB_DECIDE_MOTION_MODEL: before = the PREDICTED pose (SetPose at :866 ran) and the search's slots.  nmatches < 20 -> ok
 *             = 0, final = before (PoseOptimization did not run); else ok = nmatches_map >= 10, final = opt.  d_retry[t] = nmatches
 *             < 20 when after_retry == 0 (the first search's verdict: the caller searches again with 2 * th and decides again with
 *             after_retry = 1), 0 when after_retry != 0.
 *         PGORB_DECIDE_LOCAL_MAP: d_kp_point_opt / d_outlier = PoseOptimization's (discard_outliers = 0).  d_found[p] += 1 (NULL =
 *             not carried) for every slot with a point and no outlier flag, the atomics of increase_visible; d_inliers[t] =
 *             mnMatchesInliers = those whose point has d_point_has_obs; ok = !(mnId < mnLastRelocFrameId + mMaxFrames && inliers <
 *             50) && inliers >= 30; final = opt.  d_inliers is written in this mode only, d_retry in MOTION_MODEL only.
 *       A tracker with d_run[t] == 0 gets d_ok = 0 and nothing else is read, counted or written, in every mode.
 *       INTEGER WIDTHS (include/Tracking.h, include/Frame.h): mnId is long unsigned int, mnLastRelocFrameId and mnLastKeyFrameId
 *       unsigned int, mMaxFrames and mMinFrames int.  Every `id + frames` sum is therefore formed in 32-bit UNSIGNED arithmetic (the
 *       int converts to unsigned) and WRAPS modulo 2^32, and only then is widened to 64 bits for the comparison with mnId.
 *   pgorb_track_counters   one tracker's scalar members: frame_id = mCurrentFrame.mnId (the caller's to set per frame),
 *       last_reloc_frame_id = mnLastRelocFrameId, last_kf_frame_id = mnLastKeyFrameId, max_frames / min_frames = mMaxFrames /
 *       mMinFrames, nkfs = mpMap->KeyFramesInMap(), ref_kf = mpReferenceKF (a frame index), next_kf_id = KeyFrame::nNextId, and the
 *       local mapper's answers as bytes: stopped = isStopped(), stop_requested = stopRequested(), accept_keyframes =
 *       AcceptKeyFrames(), set_not_stop_ok = what SetNotStop(true) would return.
 *   pgorb_track_finish_batch_device   the tail of Track() (:445-476) for the trackers with d_ok, a workgroup per tracker, in the
 *       reference's order.  (a) :445-454: a slot whose point has d_point_has_obs == 0 becomes -1 and its d_outlier flag is cleared
 *       (d_outlier is in/out).  (b) NeedNewKeyFrame, monocular: false when stopped or stop_requested, or when mnId <
 *       mnLastRelocFrameId + mMaxFrames && nkfs > max_frames; nMinObs = nkfs <= 2 ? 2 : 3; nRefMatches = TrackedMapPoints(nMinObs) of
 *       row counters.ref_kf of d_kf_point: the slots whose point is in range, not bad and has at least nMinObs LIVE observations (a
 *       ref_kf out of range: 0); c1a = mnId >= mnLastKeyFrameId + mMaxFrames; c1b = mnId >= mnLastKeyFrameId + mMinFrames &&
 *       accept_keyframes; c1c is false for monocular; c2 = (float)inliers < (float)nRefMatches * 0.9f && inliers > 15 -- the int
 *       converts to float and the product is ONE FLOAT product, not double; the result is accept_keyframes when (c1a || c1b) && c2.
 *       d_interrupt_ba[t] = 1 when the condition held and accept_keyframes was 0: InterruptBA() at :1038, reported, not acted on.
 *       (c) CreateNewKeyFrame when (b) said yes and set_not_stop_ok: a key frame IS a frame of the batch, so the tracker's frame f
 *       becomes it: d_kf_point[f] = the slots as they stand now (outlier slots still present, "so that bundle adjustment will
 *       finally decide"), d_kf_pose[f] = d_pose_final[t], d_kf_id[f] = next_kf_id; then next_kf_id += 1, ref_kf = f,
 *       last_kf_frame_id = (uint32_t)frame_id, nkfs += 1.  ProcessNewKeyFrame's edits are pgorb_map_edits_from_keyframe_device with kf
 *       = d_new_kf[t].  (d) :472-476: d_kp_point_out = the slots with every outlier slot -1: the next frame's d_last_point.  Outputs
 *       per tracker: d_ref_kf_out = mpReferenceKF as pgorb_track_commit_batch_device takes it, d_new_kf = f or -1, d_interrupt_ba.
 *       A tracker without d_ok: d_kp_point_out = d_kp_point, d_ref_kf_out = counters.ref_kf, d_new_kf = -1, d_interrupt_ba = 0,
 *       nothing else written.  TWO TRACKERS OF ONE CALL MUST NOT NAME THE SAME FRAME ROW, and no tracker's ref_kf may be a frame row of
 *       the call (both would race on d_kf_point; the host form refuses them, this form does not look).  The counts are wave
 *       reductions and one LDS step, the decision is one lane's, the rows are copied by all lanes.
 *   pgorb_scene_median_depth_batch_device   KeyFrame::ComputeSceneMedianDepth(q) for every entry of d_kf [nlist]; an entry of -1
 *       (or out of range) writes nothing, so the d_neigh [nkf][max_neigh] of pgorb_create_new_map_points_batch_device can be passed
 *       flat with nlist = nkf * max_neigh and d_median_depth IS its d_median_depth.  Over every slot with a point in range -- NO
 *       isBad() test, as in the reference -- z = (float)(Rcw2.dot(x3Dw) + zcw): Mat::dot on CV_32F is a double sum from 0 in
 *       row-major order of the widened products, zcw is widened and added in double, and the sum is rounded to float once.  The
 *       result is the element at index (count - 1) / q (integer division) of the ascending order.  count == 0 is an out-of-bounds
 *       read in the reference: here -1.0f with PGORB_DEPTH_EMPTY in d_status.  A NaN depth makes std::sort undefined: here -1.0f with
 *       PGORB_DEPTH_NAN.  A zero of either sign is returned as +0.0f: operator< cannot tell them apart and std::sort is not stable,
 *       so which zero the reference returns is unspecified -- the one place where it is.  A workgroup per entry: the depths as
 *       order-preserving uint32 keys in LDS (cap_per_frame * 4 + 4128 bytes), then an exact radix select in four 8-bit histogram
 *       passes, a histogram per wave merged by one step (equal depths contend inside one wave only); no sort, no rank count.
 *   pgorb_scale_initial_map_device   CreateInitialMapMonocular, :684-709.  medianDepth = ComputeSceneMedianDepth(2) of kf_ini as above,
 *       invMedianDepth = 1.0f / medianDepth (float).  d_info [PGORB_DECIDE_INFO] = (status, the median's float bits,
 *       TrackedMapPoints(1) of kf_cur, points scaled); status = PGORB_DECIDE_WRONG_INIT | PGORB_DEPTH_* when medianDepth < 0 (EMPTY and
 *       NAN give -1) || tracked < 100: NOTHING else is written then (the reference resets).  Otherwise kf_cur's translation column is
 *       multiplied by invMedianDepth -- a float product: the MatExpr scale forms (double)t * (double)inv, exact in double, and rounds
 *       it to float, the same value -- and SetPose gives Ow = -Rcw.t()*tcw as everywhere else; then pos of every point in kf_ini's
 *       slots is multiplied the same way, ONCE PER SLOT THAT HOLDS IT (a point in two slots is scaled twice, as the loop at :702-709
 *       does), bad or not: slot counts by integer atomics in scratch, then a thread per point that multiplies that many times.  A
 *       median of +0 gives inf, as in the reference.  One workgroup, then a thread per slot and a thread per point; the median
 *       travels in d_info, no host round trip.
 *   pgorb_check_replaced / pgorb_increase_visible / pgorb_query_seen_from_outliers / pgorb_track_decide / pgorb_track_finish /
 *   pgorb_scene_median_depth / pgorb_scale_initial_map   the same flat arrays in host memory, checked on the host before anything
 *       else, byte for byte equal to the device forms (bytes a device form does not write keep their values).  PGORB_E_ARG: a negative
 *       count, a NULL array (every array is required here, except frame, run, modes, point_bad, point_has_obs and obs_live), a
 *       frame's count outside [0, cap_per_frame], a tracker's frame out of range, a slot or replacement outside [-1, npoints), a query
 *       outside [0, npoints), a query count outside [0, qcap], an unknown mode, q < 1, obs_start not rising from 0 to nobs, a live
 *       observation naming a frame out of range, two trackers on one frame row, a ref_kf out of range or equal to a tracker's frame
 *       row, a list entry outside [-1, nframes), kf_ini or kf_cur out of range or equal.  pgorb_track_finish returns the number of key
 *       frames made, pgorb_scale_initial_map the number of points scaled (0 with PGORB_DECIDE_WRONG_INIT), the others 0.
 * Still left to the caller: the relocalisation bookkeeping (Relocalization itself and mnLastRelocFrameId), System::Reset, the stereo /
 * RGB-D branches, localisation mode (mbOnlyTracking, mbVO), mCurrentFrame.mnId, and the table append of CreateNewMapPoints.
 * Limits (PGORB_E_LIMIT): ntrack <= PGORB_TRACK_MAX, nframes <= PGORB_COVIS_MAX_KF, cap_per_frame and qcap <= 16000, nlist <=
 * PGORB_DEPTH_MAX_LIST; query_seen: npoints <= 1048576; scale_initial_map: npoints <= 2^30.  Scratch arena: query_seen ntrack *
 * ((npoints + 31) / 32 + 1) * 4 bytes, scale_initial_map npoints * 4 bytes, each rounded up to 64; the others none.  Determinism: integers
 * and correctly rounded float / double operations only (the library is built with -ffp-contract=off); the only atomics are integer
 * adds and ors, whose results no order of execution changes; a result depends on its inputs alone, not on the batch position, the
 * stream or a repeat. */
#define PGORB_DECIDE_MOTION_MODEL 0
#define PGORB_DECIDE_REFERENCE_KF 1
#define PGORB_DECIDE_LOCAL_MAP    2
#define PGORB_DECIDE_WRONG_INIT   4
#define PGORB_DECIDE_INFO         4
#define PGORB_DEPTH_EMPTY         1
#define PGORB_DEPTH_NAN           2
#define PGORB_DEPTH_MAX_LIST      262144
typedef struct pgorb_track_counters {
    uint64_t frame_id;             /* mCurrentFrame.mnId */
    uint32_t last_reloc_frame_id;  /* mnLastRelocFrameId */
    uint32_t last_kf_frame_id;     /* mnLastKeyFrameId */
    int32_t max_frames, min_frames, nkfs, ref_kf;
    uint64_t next_kf_id;           /* KeyFrame::nNextId */
    uint8_t stopped, stop_requested, accept_keyframes, set_not_stop_ok, pad[4];
} pgorb_track_counters;
int  pgorb_check_replaced(pgorb_ctx* ctx,
        int ntrack, const int32_t* n /*[nframes]*/, int nframes, int cap_per_frame, const int32_t* frame /*[ntrack] or NULL*/,
        int32_t* last_point /*[ntrack][cap_per_frame] in and out*/, int npoints, const int32_t* replaced /*[npoints]*/);
int  pgorb_check_replaced_batch_device(pgorb_ctx* ctx,
        int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame, int32_t* d_last_point, int npoints,
        const int32_t* d_replaced, void* hip_stream);
int  pgorb_increase_visible(pgorb_ctx* ctx,
        int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, const uint8_t* run /*[ntrack] or NULL*/,
        const int32_t* kp_point /*[ntrack][cap_per_frame]*/, int qcap, const int32_t* nq /*[ntrack]*/,
        const int32_t* queries /*[ntrack][qcap]*/, const uint8_t* in_view /*[ntrack][qcap]*/, int npoints, int32_t* visible /*in and out*/);
int  pgorb_increase_visible_batch_device(pgorb_ctx* ctx,
        int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame, const uint8_t* d_run,
        const int32_t* d_kp_point, int qcap, const int32_t* d_nq, const int32_t* d_queries, const uint8_t* d_in_view, int npoints,
        int32_t* d_visible, void* hip_stream);
int  pgorb_query_seen_from_outliers(pgorb_ctx* ctx,
        int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, const int32_t* kp_point,
        const uint8_t* outlier /*[ntrack][cap_per_frame] or NULL*/, const int32_t* kp_point_opt /*[ntrack][cap_per_frame] or NULL*/,
        int qcap, const int32_t* nq, const int32_t* queries, int npoints, uint8_t* query_seen /*[ntrack][qcap]*/);
int  pgorb_query_seen_from_outliers_batch_device(pgorb_ctx* ctx,
        int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame, const int32_t* d_kp_point,
        const uint8_t* d_outlier, const int32_t* d_kp_point_opt, int qcap, const int32_t* d_nq, const int32_t* d_queries, int npoints,
        uint8_t* d_query_seen, void* hip_stream);
int  pgorb_track_decide(pgorb_ctx* ctx,
        int ntrack, int mode, const int32_t* modes /*[ntrack] or NULL*/, int after_retry, const int32_t* n, int nframes,
        int cap_per_frame, const int32_t* frame, const uint8_t* run, const int32_t* nmatches, const int32_t* nmatches_map /*[ntrack]*/,
        const pgorb_kf_pose* pose_before /*[ntrack]*/, const int32_t* kp_point_before, const pgorb_kf_pose* pose_opt,
        const int32_t* kp_point_opt, const uint8_t* outlier, int npoints, const uint8_t* point_has_obs, int32_t* found /*in and out*/,
        const pgorb_track_counters* counters /*[ntrack]*/, uint8_t* ok, int32_t* inliers, uint8_t* retry /*[ntrack]*/,
        pgorb_kf_pose* pose_final /*[ntrack]*/, int32_t* kp_point_final /*[ntrack][cap_per_frame]*/);
int  pgorb_track_decide_batch_device(pgorb_ctx* ctx,
        int ntrack, int mode, const int32_t* d_mode, int after_retry, const int32_t* d_n, int nframes, int cap_per_frame,
        const int32_t* d_frame, const uint8_t* d_run, const int32_t* d_nmatches, const int32_t* d_nmatches_map,
        const pgorb_kf_pose* d_pose_before, const int32_t* d_kp_point_before, const pgorb_kf_pose* d_pose_opt,
        const int32_t* d_kp_point_opt, const uint8_t* d_outlier, int npoints, const uint8_t* d_point_has_obs, int32_t* d_found,
        const pgorb_track_counters* d_counters, uint8_t* d_ok, int32_t* d_inliers, uint8_t* d_retry, pgorb_kf_pose* d_pose_final,
        int32_t* d_kp_point_final, void* hip_stream);
int  pgorb_track_finish(pgorb_ctx* ctx,
        int ntrack, const int32_t* n, int nframes, int cap_per_frame, const int32_t* frame, const uint8_t* ok, const int32_t* inliers,
        pgorb_track_counters* counters /*in and out*/, const pgorb_kf_pose* pose_final, const int32_t* kp_point,
        uint8_t* outlier /*in and out*/, int npoints, const uint8_t* point_bad, const uint8_t* point_has_obs,
        const int32_t* obs_start /*[npoints + 1]*/, const int32_t* obs_frame, int nobs, const uint8_t* obs_live,
        int32_t* kf_point /*[nframes][cap_per_frame]*/, pgorb_kf_pose* kf_pose /*[nframes]*/, uint64_t* kf_id /*[nframes]*/,
        int32_t* kp_point_out /*[ntrack][cap_per_frame]*/, int32_t* ref_kf_out, int32_t* new_kf, uint8_t* interrupt_ba /*[ntrack]*/);
int  pgorb_track_finish_batch_device(pgorb_ctx* ctx,
        int ntrack, const int32_t* d_n, int nframes, int cap_per_frame, const int32_t* d_frame, const uint8_t* d_ok,
        const int32_t* d_inliers, pgorb_track_counters* d_counters, const pgorb_kf_pose* d_pose_final, const int32_t* d_kp_point,
        uint8_t* d_outlier, int npoints, const uint8_t* d_point_bad, const uint8_t* d_point_has_obs, const int32_t* d_obs_start,
        const int32_t* d_obs_frame, int nobs, const uint8_t* d_obs_live, int32_t* d_kf_point, pgorb_kf_pose* d_kf_pose,
        uint64_t* d_kf_id, int32_t* d_kp_point_out, int32_t* d_ref_kf_out, int32_t* d_new_kf, uint8_t* d_interrupt_ba, void* hip_stream);
int  pgorb_scene_median_depth(pgorb_ctx* ctx,
        int nlist, const int32_t* kf /*[nlist]*/, int q, const int32_t* kf_point, const int32_t* n, int nframes, int cap_per_frame,
        const pgorb_kf_pose* pose /*[nframes]*/, int npoints, const pgorb_map_point* points, float* median_depth /*[nlist]*/,
        int32_t* status /*[nlist]*/);
int  pgorb_scene_median_depth_batch_device(pgorb_ctx* ctx,
        int nlist, const int32_t* d_kf, int q, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame,
        const pgorb_kf_pose* d_pose, int npoints, const pgorb_map_point* d_points, float* d_median_depth, int32_t* d_status,
        void* hip_stream);
int  pgorb_scale_initial_map(pgorb_ctx* ctx,
        int kf_ini, int kf_cur, const int32_t* kf_point, const int32_t* n, int nframes, int cap_per_frame,
        pgorb_kf_pose* pose /*[nframes] in and out*/, int npoints, pgorb_map_point* points /*in and out: pos*/, const uint8_t* point_bad,
        const int32_t* obs_start, const int32_t* obs_frame, int nobs, const uint8_t* obs_live, int32_t* info /*[PGORB_DECIDE_INFO]*/);
int  pgorb_scale_initial_map_device(pgorb_ctx* ctx,
        int kf_ini, int kf_cur, const int32_t* d_kf_point, const int32_t* d_n, int nframes, int cap_per_frame, pgorb_kf_pose* d_pose,
        int npoints, pgorb_map_point* d_points, const uint8_t* d_point_bad, const int32_t* d_obs_start, const int32_t* d_obs_frame,
        int nobs, const uint8_t* d_obs_live, int32_t* d_info, void* hip_stream);

/* ---- ORB vocabulary (DBoW2 TemplatedVocabulary<FORB::TDescriptor, FORB>) -----------------
 *   pgorb_vocab_load_text     ORBVocabulary(text_file) -> TemplatedVocabulary::loadFromTextFile
 *                             thirdparty/orb-slam2/src/ORBVocabulary.cc:7-9,
 *                             thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1337-1420
 *   pgorb_bow_transform*      TemplatedVocabulary::transform(feature, word_id, weight, nid,
 *                             levelsup)  TemplatedVocabulary.h:1217-1259 for every feature
 *   pgorb_bow_vectors         the accumulation part of transform(features, BowVector&,
 *                             FeatureVector&, levelsup)  TemplatedVocabulary.h:1126-1194 with
 *                             BowVector::addWeight/normalize (BowVector.cpp:34-84) and
 *                             FeatureVector::addFeature (FeatureVector.cpp:31-45), called from
 *                             Frame::ComputeBoW (thirdparty/orb-slam2/src/Frame.cc:399-406)
 * A vocabulary is a flat little-endian blob (layout in pilotguru_amd/vocab.py and bow.hip) so
 * that one rank can parse it and broadcast it to its peers with a single RCCL broadcast.
 * Deviation from the reference loader: empty lines are skipped (the reference appends a bogus
 * root child with an uninitialised descriptor for a trailing newline). */
typedef struct pgorb_vocab pgorb_vocab;
int  pgorb_vocab_load_text(const char* path, pgorb_vocab** out);
/* As pgorb_vocab_load_text, through a binary cache `<path>.pgvoc` beside the text file (header: the text file's size and
 * modification time; then the blob): a matching cache is loaded instead of parsing the text, anything else parses and rewrites
 * the cache (failures to write are ignored).  *from_cache (may be NULL): 1 when the cache was used. */
int  pgorb_vocab_load_cached(const char* path, pgorb_vocab** out, int* from_cache);
int  pgorb_vocab_from_blob(const void* blob, int64_t nbytes, pgorb_vocab** out);   /* copies */
int  pgorb_vocab_blob(const pgorb_vocab* v, const void** blob, int64_t* nbytes);
int  pgorb_vocab_info(const pgorb_vocab* v, int* k, int* L, int* nnodes, int* nwords,
                      int* scoring, int* weighting);
void pgorb_vocab_free(pgorb_vocab* v);
/* Make a vocabulary resident on the context's GPU (host blob: H2D copy; device blob, e.g. the
 * receive buffer of the broadcast: D2D copy on `hip_stream`). */
int  pgorb_vocab_upload(pgorb_ctx* ctx, const pgorb_vocab* v);
int  pgorb_vocab_upload_device(pgorb_ctx* ctx, const void* d_blob, int64_t nbytes, void* hip_stream);
/* ---- The vocabulary on every GPU of the node: ONE RCCL broadcast over xGMI --------------------------------------------
 * Reference: the single process loads the vocabulary once and shares it with every System by pointer
 * (src/optical_trajectories.cc:87-94, thirdparty/orb-slam2/src/ORBVocabulary.cc:7-9).  With one extractor context per
 * GPU the pointer share becomes one ncclBroadcast of the flat blob, issued from librccl directly (csrc/comm.hip; the
 * library is opened on first use).  It is the only collective of the path: frames / rides are sharded, nothing else
 * is exchanged.
 *   pgorb_comm_create_local   ONE process, one host thread per device (optical_trajectories --devices=0,1,...): the
 *                             group's ranks are the DISTINCT devices of ctxs[0..nctx) (ncclCommInitAll); contexts
 *                             that share a device share its rank and receive by a device-to-device copy.
 *   pgorb_comm_unique_id /    one PROCESS per GPU (bench.py under torch.distributed.run): rank 0 makes the 128-byte
 *   pgorb_comm_create_rank    id, the launcher's control plane hands it to the other ranks, each calls create_rank
 *                             (ncclCommInitRank; collective over the ranks).
 *   pgorb_vocab_broadcast     local form: `root` indexes ctxs, `v` = the parsed vocabulary.  Rank form: `root` is a
 *                             rank, `v` is read on that rank only (NULL elsewhere; the byte count travels first).
 *                             The receive buffer is the context's own vocabulary arena; every receiver validates
 *                             the blob's structure on its device before the vocabulary counts as resident.
 *                             *seconds (may be NULL): wall time of the collective alone.
 *   pgorb_comm_library        which librccl the library resolved (the file ncclGetUniqueId lives in).  The library asks
 *                             the loader for a librccl the PROCESS already holds first (RTLD_NOLOAD: under
 *                             torch.distributed that is torch's bundled copy) and loads one by name only when there is
 *                             none, so that one process never runs two RCCLs.  *preloaded (may be NULL) = 1 when it was
 *                             already mapped.  Returns 0, or PGORB_E_HIP with the loader's message in `path`. */
#define PGORB_COMM_ID_BYTES 128
typedef struct pgorb_comm pgorb_comm;
int  pgorb_comm_library(char* path, int cap, int* preloaded);
int  pgorb_comm_unique_id(void* id /*[PGORB_COMM_ID_BYTES]*/);
int  pgorb_comm_create_local(pgorb_ctx* const* ctxs, int nctx, pgorb_comm** out);
int  pgorb_comm_create_rank(pgorb_ctx* ctx, int rank, int nranks, const void* id, pgorb_comm** out);
int  pgorb_comm_ranks(const pgorb_comm* comm);
int  pgorb_vocab_broadcast(pgorb_comm* comm, int root, const pgorb_vocab* v, double* seconds);
void pgorb_comm_destroy(pgorb_comm* comm);
/* Per-feature word id, word weight and the ancestor node at level L - levelsup (0 = root).
 * Host buffers / device buffers + stream. */
int  pgorb_bow_transform(pgorb_ctx* ctx, const uint8_t* desc, int n, int levelsup,
                         uint32_t* word, double* weight, uint32_t* node);
int  pgorb_bow_transform_device(pgorb_ctx* ctx, const uint8_t* d_desc, int n, int levelsup,
                                uint32_t* d_word, double* d_weight, uint32_t* d_node,
                                void* hip_stream);
/* Host: BowVector (ascending word ids, L1-normalised when the scoring type says so) and
 * FeatureVector (ascending node ids, feature indices in feature order) from the per-feature
 * results.  bow_* need n entries, fv_node/fv_start n+1 entries, fv_feat n entries.
 * scoring: 0 = L1_NORM ... (BowVector.h:36-53); weighting 0 = TF_IDF, 1 = TF. */
int  pgorb_bow_vectors(int n, const uint32_t* word, const double* weight, const uint32_t* node,
                       int scoring, int weighting,
                       uint32_t* bow_id, double* bow_val, int* n_bow,
                       uint32_t* fv_node, int32_t* fv_start, uint32_t* fv_feat, int* n_fv);
/* L1Scoring::score(v1, v2), ScoringObject.cpp:23-60 (host). */
double pgorb_bow_score_l1(const uint32_t* id1, const double* val1, int n1,
                          const uint32_t* id2, const double* val2, int n2);

/* ---- Place recognition: KeyFrameDatabase candidate queries (csrc/place.hip) ---------------------------------------------------
 * Reference (thirdparty/orb-slam2): Tracking::Relocalization asks KeyFrameDatabase::DetectRelocalizationCandidates
 * (src/Tracking.cc:1330, src/KeyFrameDatabase.cc:212-310); LoopClosing::DetectLoop takes minScore as the lowest score against
 * the connected key frames (src/LoopClosing.cc:120-141) and asks DetectLoopCandidates (src/KeyFrameDatabase.cc:89-210).
 *
 * BowVector table: frame f's BowVector is d_bow_id[f * cap .. f * cap + d_nbow[f]) (ascending word ids, no repeats) with its
 * values at the same places of d_bow_val -- what TemplatedVocabulary::transform (TemplatedVocabulary.h:1126-1194) leaves in
 * mBowVec.
 *
 * pgorb_bow_vectors_batch_device  the BowVector of every frame from pgorb_bow_transform_device's per-feature results
 *   ([nframes][cap_per_frame], the first d_n[f] of each row), bit-equal to pgorb_bow_vectors: features with weight <= 0 are
 *   skipped, a word's weights are added in feature order, the norm is the running double sum of fabs in ascending word order, every
 *   value is divided by it when it is > 0.  One workgroup per frame: a stable sort by word id (ranks by counting on LDS), then
 *   one sequential sum per word and one for the norm.  The context's vocabulary must be L1_NORM with TF_IDF or TF (else
 *   PGORB_E_ARG); at most 8192 features per frame (PGORB_E_LIMIT).
 * pgorb_bow_score_l1_batch_device  d_score[p] = L1Scoring::score(frame d_pair_a[p], frame d_pair_b[p]) (ScoringObject.cpp:23-60),
 *   bit-equal to pgorb_bow_score_l1: one wave per pair, ONE running double sum over the common words in ascending word order.
 *   This is the minScore loop of LoopClosing.cc:124-138; the caller takes the minimum over its non-bad connected key frames.
 *   A pair index outside [0, nframes) reads as an empty vector.
 *
 * The two queries, over one table of frames:
 *   d_in_db [nframes] u8      whether the frame is in the database.  Members must appear in the table in add() order
 *                             (KeyFrameDatabase.cc:53-59 appends a key frame to every one of its words' lists, so all inverted
 *                             lists share that order); other frames may sit anywhere and never share words.
 *   d_neigh [nframes][10]     GetBestCovisibilityKeyFrames(10) in order, padded with -1; -1 and out-of-range indices are skipped
 *   d_query [nq]              frame indices of the queries (out of range: an empty query)
 *   d_score_state [nframes]   relocalisation form: the stored mRelocScore of every frame on entry; NULL = 0.0f.  The reference
 *                             never initialises it (KeyFrame.cc:138), so ITS value for a never-scored key frame is
 *                             indeterminate; here it is what the caller passes.  The loop form takes no state: every
 *                             mLoopScore it reads was written by the same query.
 *   loop form only            d_min_score [nq]; the connected sets (pKF->GetConnectedKeyFrames()) as CSR d_conn_start [nq + 1]
 *                             into d_conn [nconn], in any order
 *   d_cand [nq][ccap], d_ncand [nq]   the candidates in the reference's order; d_ncand is the full count, only the first ccap
 *                             are written
 *   d_common [nq][nframes]    (may be NULL) common words; 0 = the frame is not in lKFsSharingWords
 *   d_score [nq][nframes]     (may be NULL) the stored scores afterwards: the state on entry, overwritten where a frame was scored
 *   d_stats [nq][3]           (may be NULL) length of lKFsSharingWords, maxCommonWords, nscores
 * Decomposition (proved in DESIGN.md section 4).  lKFsSharingWords (:99-117, :220-236) is the database members with a common word
 * -- the loop form drops the connected key frames -- sorted by (smallest common word, table index), each with its number of
 * common words.  k_place_overlap, one wave per (query, key frame), finds count, smallest common word and the score (one running
 * double sum, rounded to float as `float si`).  k_place_decide, one workgroup per query: minCommonWords = (int)(max * 0.8f); a
 * frame is scored iff count > minCommonWords; an entry of lScoreAndMatch (every scored frame; loop form: si >= minScore) reads
 * only stored scores, so every entry accumulates on its own over its first 10 neighbours in order, in float, a strictly larger
 * score moving pBestKF.  Relocalisation counts a neighbour with mnRelocQuery == id, i.e. every sharing frame: one that was not
 * scored gives its STALE score from d_score_state.  The loop form also asks mnLoopWords > minCommonWords, so its reads are always
 * fresh.  bestAccScore starts at 0 / minScore; entries with acc > 0.75f * best emit their pBestKF in list order, first
 * occurrence only.
 * Each query equals the reference called on the state it was given.  The reference runs queries one after another and the stale
 * read sees earlier queries' scores: ordering queries that matter to each other is the caller's job -- feed d_score row q as the
 * next call's d_score_state.  The batched forms do not check their inputs, but no index can cause an out-of-bounds access.
 * Limits: PGORB_E_LIMIT above 65 536 frames, and above 65 535 queries in one batch.  Every per-query list lives in a global slab
 * of 40 bytes per (query, frame) taken from the context's matcher scratch arena -- 40 * nq * nframes bytes, 167 MB for 64 queries
 * over 65 536 frames --, so the scored set has no LDS bound, and what bounds nq is that arena's allocation (PGORB_E_HIP when the
 * device cannot give it; split the batch).  The final ordering of the emitted candidates is by counting, quadratic in THEIR
 * number.  The single host calls pad the CSR BowVectors to the longest one and refuse a padded table of more than 2^28 entries
 * (nkf * longest BowVector) with PGORB_E_LIMIT.
 * A context whose uploaded vocabulary is not L1_NORM refuses these calls (PGORB_E_ARG); without a vocabulary they run on the
 * caller's BowVectors.
 *
 * Single host calls: BowVectors as CSR (bow_start [nkf + 1], bow_id, bow_val), neighbours as CSR (neigh_start [nkf + 1], neigh,
 * at most 10 each), one query; staged as a one-query batch.  score_state [nkf] (may be NULL = zeros) is in/out; the loop form
 * returns its stored scores in `score` (may be NULL).  They return the full candidate count (>= 0; the first ccap are written) and
 * check their inputs: PGORB_E_ARG for unsorted or repeated word ids, indices out of range, a neighbour list longer than 10, start
 * arrays that do not begin at 0 or that decrease. */
int  pgorb_bow_vectors_batch_device(pgorb_ctx* ctx, const uint32_t* d_word, const double* d_weight, const int32_t* d_n, int nframes,
                                    int cap_per_frame, uint32_t* d_bow_id, double* d_bow_val, int32_t* d_nbow, void* hip_stream);
int  pgorb_bow_score_l1_batch_device(pgorb_ctx* ctx, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nframes,
                                     int cap, const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs, double* d_score,
                                     void* hip_stream);
int  pgorb_detect_relocalization_candidates_batch_device(pgorb_ctx* ctx, const uint32_t* d_bow_id, const double* d_bow_val,
                                                         const int32_t* d_nbow, int nframes, int cap, const uint8_t* d_in_db,
                                                         const int32_t* d_neigh, const int32_t* d_query, int nq,
                                                         const float* d_score_state, int32_t* d_cand, int ccap, int32_t* d_ncand,
                                                         int32_t* d_common, float* d_score, int32_t* d_stats, void* hip_stream);
int  pgorb_detect_loop_candidates_batch_device(pgorb_ctx* ctx, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow,
                                               int nframes, int cap, const uint8_t* d_in_db, const int32_t* d_neigh,
                                               const int32_t* d_query, int nq, const float* d_min_score, const int32_t* d_conn_start,
                                               const int32_t* d_conn, int nconn, int32_t* d_cand, int ccap, int32_t* d_ncand,
                                               int32_t* d_common, float* d_score, int32_t* d_stats, void* hip_stream);
int  pgorb_detect_relocalization_candidates(pgorb_ctx* ctx, int nkf, const int32_t* bow_start, const uint32_t* bow_id,
                                            const double* bow_val, const uint8_t* in_db, const int32_t* neigh_start, const int32_t* neigh,
                                            int query, float* score_state, int32_t* cand, int ccap, int32_t* common, int32_t* stats);
int  pgorb_detect_loop_candidates(pgorb_ctx* ctx, int nkf, const int32_t* bow_start, const uint32_t* bow_id, const double* bow_val,
                                  const uint8_t* in_db, const int32_t* neigh_start, const int32_t* neigh, int query, float min_score,
                                  const int32_t* conn, int nconn, int32_t* cand, int ccap, int32_t* common, float* score,
                                  int32_t* stats);

/* ---- after the path: what TrackImageSequence does to the finished trajectory ----
 * Host functions, double precision, no context needed (the reference runs them once per segment on
 * the CPU).  Quaternions are (w, x, y, z) like the JSON; all arrays are row-major.
 *   pgorb_smooth_heading_directions  SmoothHeadingDirections(trajectory, sigma)  src/slam/smoothing.cc:11-47
 *                                    (cv::getGaussianKernel(4*sigma+1, sigma), cv::sepFilter2D with
 *                                    BORDER_REPLICATE along the trajectory, renormalisation); sigma <= 0 is the
 *                                    reference's CHECK failure -> PGORB_E_ARG
 *   pgorb_smooth_time_series         SmoothTimeSeries(values, timestamps, targets, sigma)  smoothing.cc:57-97
 *   pgorb_trajectory_pca             TrajectoryToPCA  src/slam/track_image_sequence.cc:16-29: cv::PCA with
 *                                    CV_PCA_DATA_AS_COL over the translations; eigenvectors[3][3] (rows, by
 *                                    descending eigenvalue), eigenvalues[3], mean[3] (may be NULL).  The plane of
 *                                    :92 is the first two rows; :83-90 drops the trajectory when
 *                                    eigenvalues[2] > eigenvalues[1] * 1e-2.  n < 3 -> PGORB_E_LIMIT
 *   pgorb_project_directions         ProjectDirections  src/slam/horizontal_flatten.cc:7-30 -> dirs[n][2]
 *   pgorb_project_translations       ProjectTranslations  horizontal_flatten.cc:32-43 (in place)
 *   pgorb_turn_angles                Projected2DDirectionsToTurnAngles  horizontal_flatten.cc:45-63 */
int  pgorb_smooth_heading_directions(double* quat_wxyz /* [n][4] in/out */, int n, int sigma);
int  pgorb_smooth_time_series(const double* values, const double* times, int n,
                              const double* targets, int m, double sigma, double* out /* [m] */);
int  pgorb_trajectory_pca(const double* translations /* [n][3] */, int n,
                          double* eigenvectors /* [3][3] */, double* eigenvalues /* [3] */, double* mean /* [3] or NULL */);
int  pgorb_project_directions(const double* quat_wxyz, int n, const double* plane /* [2][3] */, double* dirs /* [n][2] */);
int  pgorb_project_translations(double* translations /* [n][3] in/out */, int n, const double* plane);
int  pgorb_turn_angles(const double* dirs /* [n][2] */, int n, double* turn /* [n] */);

/* ---- fit_motion's velocity calibration (BASELINE configs[4]), K9 calib.hip ----
 * Inputs are the three recorder series as arrays: GPS speed [n_gps] + time, gyroscope rates
 * [n_rot][3] (rad/s) + time, accelerations [n_acc][3] + time; times in microseconds, increasing.
 *   pgorb_fit_num_windows        number of sliding windows = ceil(n_gps / locations_shift_step)
 *                                (the loop of src/fit_motion.cc:173-176)
 *   pgorb_fit_velocity_windows   for every window: AccelerometerCalibrator over the window's GPS fixes
 *                                (src/calibration/velocity.cc:30-180) minimised from x = 0 with
 *                                LBFGSpp::LBFGSSolver (thirdparty/LBFGS/LBFGS.h:78-181, epsilon 1e-5,
 *                                max_iterations = optimization_iters; fit_motion.cc:163-190).  All windows
 *                                run concurrently on the GPU, one lane each.  x[w][9] = global bias, local
 *                                bias, initial velocity; residual[w] = loss; niter[w] = iterations, or -2 / -3
 *                                where LBFGSpp would throw (line-search step below 1e-20 / above 1e20).
 *   pgorb_calibrator_eval        AccelerometerCalibrator::operator() (velocity.cc:182-194) of ONE calibrator
 *                                at n_points parameter vectors xin[n_points][9] -> fx[n_points], grad[n_points][9]
 *   pgorb_fit_motion_velocities  ComputeAndSaveForwardVelocitiesFromImu (fit_motion.cc:151-290) up to the JSON:
 *                                window fits on the GPU, then IntegrateTrajectory, per-sample averaging,
 *                                SmoothTimeSeries and the forward axis on the host.  out_* need n_rot + n_acc entries. */
/*   pgorb_principal_rotation_axes         GetPrincipalRotationAxes (src/calibration/rotation.cc:16-57): gyroscope
 *                                         rates integrated over intervals of integration_interval_usec, cv::PCA over
 *                                         the quaternion vector parts; eigenvectors[3][3] rows by descending
 *                                         eigenvalue, row 0 = the vehicle's vertical axis (fit_motion.cc:322-329).
 *                                         Fewer than 3 integrated intervals -> PGORB_E_LIMIT.  Host.
 *   pgorb_angular_velocities_around_axis  GetAngularVelocitiesAroundAxisDirect (rotation.cc:111-129) = the steering
 *                                         output of fit_motion (fit_motion.cc:130-148); axis must have norm 1 +- 1e-2. Host. */
int  pgorb_principal_rotation_axes(const double* rotations /* [n][3] */, const int64_t* rot_time_usec, int n,
                                   int64_t integration_interval_usec, double* eigenvectors /* [3][3] */);
int  pgorb_angular_velocities_around_axis(const double* rotations, int n, const double* axis /* [3] */, double* out /* [n] */);
/*   pgorb_kahan_sum                       KahanSum<T>::add over n vectors of dim components (include/math/math.hpp:8-25),
 *                                         the accumulator of fit_motion's forward-axis estimate.  Host. */
int  pgorb_kahan_sum(const double* values /* [n][dim] */, int n, int dim, double* sum /* [dim] */);
int  pgorb_fit_num_windows(int n_gps, int locations_shift_step);
int  pgorb_fit_velocity_windows(pgorb_ctx* ctx, const double* gps_velocity, const int64_t* gps_time_usec, int n_gps,
                                const double* rotations, const int64_t* rot_time_usec, int n_rot,
                                const double* accelerations, const int64_t* acc_time_usec, int n_acc,
                                int locations_batch_size, int locations_shift_step, int optimization_iters,
                                double* x /* [nw][9] */, double* residual /* [nw] */, int32_t* niter /* [nw] */);
int  pgorb_calibrator_eval(pgorb_ctx* ctx, const double* gps_velocity, const int64_t* gps_time_usec, int n_gps,
                           const double* rotations, const int64_t* rot_time_usec, int n_rot,
                           const double* accelerations, const int64_t* acc_time_usec, int n_acc,
                           const double* xin, int n_points, double* fx, double* grad);
int  pgorb_fit_motion_velocities(pgorb_ctx* ctx, const double* gps_velocity, const int64_t* gps_time_usec, int n_gps,
                                 const double* rotations, const int64_t* rot_time_usec, int n_rot,
                                 const double* accelerations, const int64_t* acc_time_usec, int n_acc,
                                 const double* vertical_axis /* [3] */, int locations_batch_size, int locations_shift_step,
                                 int optimization_iters, double post_smoothing_sigma_sec,
                                 double forward_axis_inference_min_velocity_m_s, double forward_axis_inference_min_rotation_rad,
                                 int64_t* out_time_usec, double* out_velocity, int* n_out, double* forward_axis /* [3] */);

/* Per-stage device timing with HIP events recorded on the launch stream around the kernel
 * groups of every *_device call: stage 0 = pyramid chain (K1, nlevels-1 launches), 1 = FAST
 * cells (K2), 2 = quadtree (K3), 3 = orientation+blur+rBRIEF (K4-6), 4 = Hamming match (K7).
 * pgorb_profile_begin arms up to max_calls calls (0 disarms); pgorb_profile_read synchronises,
 * writes the mean milliseconds per call of each stage into ms[5] and returns the number of
 * calls averaged. */
#define PGORB_NSTAGES 5
int  pgorb_profile_begin(pgorb_ctx* ctx, int max_calls);
int  pgorb_profile_read(pgorb_ctx* ctx, double* ms);

/* ---- Streamed ingest: frames that start in HOST memory --------------------------------------------------
 * Replaces the reference's frame loop around the extractor -- ImageSequenceSource::next() handing one decoded
 * frame at a time to System::TrackMonocular (src/io/image_sequence_reader.cc:138-208,
 * src/slam/track_image_sequence.cc:43-47) -- for callers whose frames are not already on the GPU.  A stream owns
 * `depth` (2..8) slots; a slot is one batch of up to `batch` w x h grey frames in PAGE-LOCKED host memory that
 * the decoder fills directly (pgorb_stream_input).  pgorb_stream_submit queues, without blocking: the upload of
 * the slot, K1..K6 on it, K7 of every frame against its predecessor (frame 0 against the last frame of the
 * previously submitted batch; after pgorb_stream_reset, or at the start, it has none and its best_idx are -1),
 * and the download of all results -- on three HIP streams, so the upload of batch i+1 and the download of
 * batch i-1 overlap the kernels of batch i.  pgorb_stream_wait blocks until the slot's results are in host
 * memory and returns the number of frames of the batch (< 0: error); the pointers stay valid until the slot is
 * submitted again: n[f] keypoints of frame f, kps[f * cap + i], desc[(f * cap + i) * 32], and for query
 * keypoint i of frame f best_idx / best / second [f * cap + i] exactly as pgorb_match_batch_device returns them.
 * One stream per context at a time; the context's other calls must not run between submit and wait. */
typedef struct pgorb_stream pgorb_stream;
int      pgorb_stream_create(pgorb_ctx* ctx, int w, int h, int batch, int depth, pgorb_stream** out);
/* The same stream for frames EXACTLY AS THE DECODER PRODUCES THEM: the reference's reader hands out RGB24 frames
 * (src/io/image_sequence_reader.cc:138-208, per-pixel copy :174-183), rotates them by the video metadata (:186-205),
 * the wrapper source flips them (:53-58, :212-222) and Tracking::GrabImageMonocular converts to grey
 * (thirdparty/orb-slam2/src/Tracking.cc:247-260) -- all on the host.  Here a slot holds src_w x src_h frames of
 * `channels` (1, 3, 4) interleaved bytes per pixel, row pitch src_w * channels, rgb_order as in
 * pgorb_extract_batch_ingest_device; rotation, flips and the grey conversion run on the device in front of K1 (one
 * pass: k_ingest / k_ingest_rows) and the extractor sees the upright (src_h x src_w for 90 / 270) grey frame.  Results,
 * matches across batch borders and the front-end stage are those of pgorb_stream_create on the host-converted frames. */
int      pgorb_stream_create_ingest(pgorb_ctx* ctx, int src_w, int src_h, int channels, int rgb_order, int rotate_degrees,
                                    int vertical_flip, int horizontal_flip, int batch, int depth, pgorb_stream** out);
void     pgorb_stream_destroy(pgorb_stream* s);                  /* pgorb_destroy(ctx) also destroys the context's live streams */
uint8_t* pgorb_stream_input(pgorb_stream* s, int slot);          /* batch * src_h * src_w * channels bytes, row pitch src_w * channels */
int      pgorb_stream_reset(pgorb_stream* s);                    /* the next batch starts a new ride */
int      pgorb_stream_submit(pgorb_stream* s, int slot, int nframes);
int      pgorb_stream_wait(pgorb_stream* s, int slot, const int32_t** n, const pgorb_keypoint** kps, const uint8_t** desc,
                           const int32_t** best_idx, const uint16_t** best, const uint16_t** second, int* cap);
/* The same stream for frames that are ALREADY RESIDENT on the device, with several batches in flight INSIDE the library
 * (round 5).  The reference's loop hands the extractor one frame after the other (Frame.cc:251-257); a caller with
 * resident frames submits batch after batch without blocking and the stream runs consecutive batches on `lanes`
 * (1..depth; 2 is what pays on an MI355X) independent extractor working sets -- lane 0 is the context itself, the others
 * are private siblings with the same parameters and options -- each on its own internal HIP stream, so that kernels of
 * neighbouring batches with different bottlenecks share the chip: K1 (HBM) beside K2 / K4-6 (VALU issue), K3 (latency),
 * K7 (matrix pipe).  Slot k runs on lane k % lanes.  Results are exactly those of the one-batch-at-a-time calls: K1..K6
 * of a batch depend on nothing outside it; what crosses batches (frame 0's match against the last frame of the
 * previously SUBMITTED batch, the front-end stage's state) is one section at the end of each batch's queue, chained in
 * submission order by an event.
 *   pgorb_stream_submit_device   d_frames: nframes grey planes (row pitch `stride`, `frame_stride` bytes apart), ready
 *                                where `hip_stream` (the caller's; NULL = the null stream) stands at the call; they
 *                                must stay valid until the slot's batch is complete (level 0 may alias them).
 *   pgorb_stream_wait_device     wait_on_host != 0: blocks until the slot's batch is complete and checks its status
 *                                word; otherwise makes `hip_stream` (NULL = the null stream, as in submit) wait for it
 *                                and returns at once.
 *                                DEVICE pointers, laid out as pgorb_stream_wait's, valid until the slot is submitted
 *                                again; with the front-end stage on, pgorb_stream_frontend_results hands out device
 *                                pointers as well.  Returns the number of frames of the batch. */
int      pgorb_stream_create_device(pgorb_ctx* ctx, int w, int h, int batch, int depth, int lanes, pgorb_stream** out);
int      pgorb_stream_submit_device(pgorb_stream* s, int slot, const uint8_t* d_frames, int nframes, int stride,
                                    int64_t frame_stride, void* hip_stream);
int      pgorb_stream_wait_device(pgorb_stream* s, int slot, int wait_on_host, void* hip_stream, const int32_t** d_n,
                                  const pgorb_keypoint** d_kps, const uint8_t** d_desc, const int32_t** d_best_idx,
                                  const uint16_t** d_best, const uint16_t** d_second, int* cap);
int      pgorb_stream_lanes(const pgorb_stream* s);
/* Optional front-end stage of the stream: what the reference's tracking thread does with every fresh Frame, run on
 * the device for the whole batch behind K7 -- Frame::AssignFeaturesToGrid with the given image bounds
 * (src/Frame.cc:234-249), ORBmatcher(nnratio, check_orientation).SearchForInitialization(previous frame, frame,
 * vbPrevMatched = the previous frame's keypoint positions, matches, window_size) as MonocularInitialization calls it
 * (Tracking.cc:583-597; frame 0 of a batch against the last frame of the previous one) and, when bow_levelsup >= 0
 * and a vocabulary is resident in the context, Frame::ComputeBoW's ORBVocabulary::transform (Frame.cc:399-406; per
 * feature word / weight / node, pgorb_bow_vectors turns them into BowVector / FeatureVector on the host).
 * Call with no batch in flight; the next batch starts a new ride.  After pgorb_stream_wait(slot):
 * pgorb_stream_frontend_results -> matches12[f * cap + i1] (-1 = none) and nmatches[f] for the pair (frame f - 1,
 * frame f) -- the first frame of a ride has no predecessor: it reports 0 matches and its matches12 row is undefined --, word / weight / node
 * [f * cap + i] (nullptr without BoW); valid until the slot is submitted again. */
int      pgorb_stream_frontend(pgorb_stream* s, float min_x, float max_x, float min_y, float max_y, int window_size,
                               float nnratio, int check_orientation, int bow_levelsup);
int      pgorb_stream_frontend_results(pgorb_stream* s, int slot, const int32_t** matches12, const int32_t** nmatches,
                                       const uint32_t** word, const double** weight, const uint32_t** node);

/* Measurement switches (no counterpart in the reference; results never depend on them -- the parity suite
 * runs under each).  Every option belongs to the CONTEXT it is set on (round 4: "matcher" / "match_mode" were process-wide
 * statics); the environment (PGORB_MATCH_POPCOUNT, PGORB_MATCH_MODE) only seeds pgorb_create.  ctx == NULL or an unknown
 * key -> PGORB_E_ARG.
 * key "matcher": 0 = the default (fp4 block-scaled MFMA for < 8192 descriptors per frame, unless PGORB_MATCH_POPCOUNT is
 * set), 1 = the ballot / popcount kernels BASELINE.json's north star describes, for every size.
 * key "match_mode": how the MFMA matcher gets its train descriptors -- -1 = chosen by the size of the launch (default), 2 = expanded
 * in LDS by 16-wave workgroups, 1 = by 4-wave workgroups, 0 = expanded into a scratch slab by a kernel of its own (rounds 1-2;
 * the slab is sized at every launch, also for streams created before the switch).
 * key "fast_tile_pitch": K2's LDS window pitch in bytes, the tile-size sweep of BASELINE.json configs[2] -- 0 = automatic
 * (48 with compile-time offsets for cells up to 36 px: the shipped shape), 48 | 64 | ... | 128 = that pitch through the
 * run-time-pitch instantiation (values below what the plan's cells need are ignored).
 * key "fast_waves_per_block": 1 (default) | 2 | 4 independent cells (waves) per K2 workgroup (measured 7 % / 15 % slower, round 5).
 * key "fast_cells_per_wave": 1 (default) ... 64 consecutive cell records a K2 wave walks, one after the other (round 5; measured
 *     slower from 2 on, profiles/r05_k2_cells_per_wave.txt: a sweep knob like the two above).
 * key "quadtree_split": K3's pass over the candidates -- 0 = inside the quadtree kernel (one launch), 1 = as a kernel of its own
 * (many small workgroups; pays for single frames and large frames), 2 = chosen per launch from the frame size and the number of
 * frames (default; the measured table is profiles/r04_k3_split_grid.txt).  PGORB_QT_SPLIT seeds it.
 * key "quadtree_threads": threads per K3 workgroup -- 0 = chosen per launch (default: 512 when the problems of a launch queue for the
 * chip or are small, 1024 when each has a CU to itself; profiles/r04_k3_threads_grid.txt), 256 | 512 | 1024 = that many.  PGORB_QT_THREADS seeds it.
 * key "fused_levels": 1 = the launch that resizes level l -> l + 1 also detects level l (csrc/fused.hip: every level read from HBM
 *     once, one wave per cell slot; bit-exact; measured SLOWER than the two launches in every form tried, profiles/r06_fused_forms.txt),
 *     0 = K1 + K2 (default).  Levels whose geometry the fused launch does not take (cells wider than 32 px, generic scale factors) run K1 + K2 either way.
 * key "fused_launches" (read only): how many levels the last batch sent through the fused launch.
 * key "pipeline_pyramid": 1 = the resize chain on a side stream beside K2, level by level (slower).
 * key "pipeline_levels": bit l set = a group of levels starts at level l; K3 / K4-6 of one group run on side streams beside K2
 * of the next (slower for every grouping measured).  0 = one launch per kernel (default).
 * key "pipeline_levels_priority": 1 = the K3 side stream is created with the highest priority (read when it is first used).
 * pgorb_get_option returns the value, or PGORB_OPTION_UNKNOWN for a null context / unknown key (-1 is a legal "match_mode"). */
#define PGORB_OPTION_UNKNOWN (-2147483647 - 1)
int  pgorb_set_option(pgorb_ctx* ctx, const char* key, int value);
int  pgorb_get_option(const pgorb_ctx* ctx, const char* key);
/* 1 when a match of `cap_per_frame` descriptors per frame takes the popcount kernels, else 0 */
int  pgorb_matcher_is_popcount(const pgorb_ctx* ctx, int cap_per_frame);

/* Host-side phases of the pgorb_extract / pgorb_extract_batch calls since the last reset, summed, in microseconds:
 * us[0] input staging + upload issue, us[1] kernel launches + download issue, us[2] wait for the GPU, us[3] results into the
 * caller's buffers.  Returns the number of calls covered; reset != 0 clears the sums (us may be NULL).  The one-frame-per-call
 * shape of the reference (Frame.cc:251-257) is measured with it: bench.py "single_frame", tools/single_frame_bench.py. */
int  pgorb_profile_host(pgorb_ctx* ctx, double* us /*[4]*/, int reset);

/* Stage taps for parity tests (host buffers, synchronous; operate on the LAST batch). */
int  pgorb_debug_level_size(const pgorb_ctx* ctx, int level, int* w, int* h);
int  pgorb_debug_level_image(pgorb_ctx* ctx, int frame, int level, uint8_t* out /* w*h */);
/* candidates of (frame, level) in device order (unordered set); x,y region-relative like
 * the reference's vToDistributeKeys (ORBextractor.cc:818-826).  Returns the count. */
int  pgorb_debug_level_candidates(pgorb_ctx* ctx, int frame, int level,
                                  int32_t* x, int32_t* y, int32_t* response, int cap);
int  pgorb_debug_level_keypoints(pgorb_ctx* ctx, int frame, int level);
/* Parity tap of the device's sin / cos contract: 64-bit checksums of pg_sincos_f over `count` consecutive
 * float bit patterns from `first_bits`, `nblocks` blocks -> out[nblocks]; compared with the oracle's for EVERY float input
 * (tests/test_gpu_parity.py::test_device_sincos_equals_the_oracle_for_every_input).  Synchronous. */
int  pgorb_debug_sincos_checksum(uint32_t first_bits, uint32_t count, int nblocks, unsigned long long* out);

/* The shared arenas of a context, read-only, for tests that keep ONE context through many kinds of call and must see when an arena
 * was reallocated (tests/test_context_session.py): address and size in bytes of arena `which` (null, 0: not allocated yet).
 * PLAN_PYR and PLAN_TABLES stand for the per-frame-size plan arenas, which make_plan sizes together. */
enum { PGORB_ARENA_STAGE_A = 0, PGORB_ARENA_PINNED = 1, PGORB_ARENA_SCRATCH = 2, PGORB_ARENA_STAGE_OUT = 3, PGORB_ARENA_XDESC = 4,
       PGORB_ARENA_OUT_BLOCK = 5, PGORB_ARENA_VOCAB = 6, PGORB_ARENA_PLAN_PYR = 7, PGORB_ARENA_PLAN_TABLES = 8 };
int  pgorb_debug_arena(const pgorb_ctx* ctx, int which, const void** ptr, int64_t* bytes);
/* How the last pgorb_extract / pgorb_extract_batch ran its kernels: 0 direct launches, 1 captured into a graph and launched,
 * 2 a replay of the captured graph; and the plan epoch (it moves with every new plan and every pgorb_set_option). */
int  pgorb_debug_host_graph(const pgorb_ctx* ctx, int* last_call, int* plan_epoch);

#ifdef __cplusplus
}
#endif
#endif
