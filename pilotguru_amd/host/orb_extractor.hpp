// orb_extractor.hpp -- C++ host-side mirror of ORB_SLAM2::ORBextractor / ORBmatcher over the
// C ABI (include/pgorb.h).  Same names, argument meaning and error behaviour as
//   thirdparty/orb-slam2/include/ORBextractor.h:44-110   (operator(), Get* accessors)
//   thirdparty/orb-slam2/include/ORBmatcher.h:40-53      (DescriptorDistance, SearchForInitialization,
//                                                          SearchForTriangulation, Fuse)
// but OpenCV-free: images are raw 8-bit planes, keypoints are pgorb_keypoint (the cv::KeyPoint
// layout), descriptors are N x 32 bytes.  INTEGRATION.md shows the cv::Mat-typed variant a
// pilotguru maintainer drops into Frame::ExtractORB.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pgorb.h"

namespace pgorb {

struct Image8 {                       // CV_8UC1 view
    const uint8_t* data = nullptr;
    int cols = 0, rows = 0, step = 0;
    bool empty() const { return !data || cols <= 0 || rows <= 0; }
};

class ORBextractor {
 public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                 int maxWidth = 1920, int maxHeight = 1080, int maxBatch = 1, int device = 0)
        : nlevels_(nlevels), scaleFactor_(scaleFactor)
    {
        pgorb_params p = {nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, maxWidth, maxHeight, maxBatch, device, 0};
        if (pgorb_create(&p, &ctx_) != PGORB_OK) throw std::runtime_error(pgorb_last_error(nullptr));
        const int n = nlevels + 1;
        mvScaleFactor.resize(n); mvInvScaleFactor.resize(n); mvLevelSigma2.resize(n); mvInvLevelSigma2.resize(n);
        pgorb_scale_tables(ctx_, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(), mvInvLevelSigma2.data());
    }
    ~ORBextractor() { pgorb_destroy(ctx_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // operator()(image, mask, keypoints, descriptors); the mask is ignored as in the reference
    // (ORBextractor.h:58); an empty image returns silently with outputs untouched (:1045).
    void operator()(const Image8& image, const Image8& /*mask*/, std::vector<pgorb_keypoint>& keypoints,
                    std::vector<uint8_t>& descriptors)
    {
        if (image.empty()) return;
        const int cap = pgorb_max_keypoints(ctx_, image.cols, image.rows);
        if (cap < 0) throw std::runtime_error("frame size unusable for the ORB cell grid");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        if (pgorb_extract(ctx_, image.data, image.cols, image.rows, image.step, keypoints.data(), descriptors.data(), cap, &n) != PGORB_OK)
            throw std::runtime_error(pgorb_last_error(ctx_));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    int GetLevels() { return nlevels_; }
    float GetScaleFactor() { return scaleFactor_; }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }
    pgorb_ctx* context() { return ctx_; }

 private:
    pgorb_ctx* ctx_ = nullptr;
    int nlevels_;
    float scaleFactor_;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// The slice of ORB_SLAM2::Frame the matcher needs (keypoints == undistorted keypoints, k1 == 0).
struct Frame {
    std::vector<pgorb_keypoint> mvKeysUndistorted;
    std::vector<uint8_t> mDescriptors;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;      // ComputeImageBounds, Frame.cc:461-466
    int N() const { return (int)mvKeysUndistorted.size(); }
};

// DBoW2::FeatureVector as CSR (what pgorb_bow_vectors returns): node ids ascending, the features of node k at
// mFeat[mStart[k] .. mStart[k + 1]).
struct FeatureVector {
    std::vector<uint32_t> mNode;
    std::vector<int32_t> mStart{0};
    std::vector<uint32_t> mFeat;
    int size() const { return (int)mNode.size(); }
};

namespace detail {
inline void checkDescriptors(const Frame& F, const char* fn)
{
    if (F.mDescriptors.size() != (size_t)F.N() * 32) throw std::invalid_argument(std::string(fn) + ": descriptors are not N x 32 bytes");
}
// what the library reads of a key frame through its pointers: N descriptors, N mask entries (or none), mStart[n] feature indices
inline void checkKeyFrame(const Frame& K, const FeatureVector& fv, const std::vector<uint8_t>& hasPoint, const char* fn)
{
    checkDescriptors(K, fn);
    if (!hasPoint.empty() && hasPoint.size() != (size_t)K.N())
        throw std::invalid_argument(std::string(fn) + ": a hasPoint mask is neither empty nor N entries long");
    if (fv.mStart.size() != fv.mNode.size() + 1 || fv.mStart.back() < 0 || fv.mFeat.size() < (size_t)fv.mStart.back())
        throw std::invalid_argument(std::string(fn) + ": FeatureVector arrays of inconsistent lengths");
}
}  // namespace detail

// The map points one Fuse call reads (include/pgorb.h): pose fields, 32-byte descriptors, bad flags (empty = none bad) and the
// observations as CSR, obsKf[obsStart[i] .. obsStart[i + 1]) = the KeyFrame::mnId of every key frame observing point i, ascending.
struct MapPointTable {
    std::vector<pgorb_map_point> points;
    std::vector<uint8_t> descriptors;
    std::vector<uint8_t> bad;
    std::vector<int32_t> obsStart{0};
    std::vector<uint64_t> obsKf;
    int size() const { return (int)points.size(); }
};

namespace detail {
// everything pgorb_fuse rejects, and the lengths it reads through its pointers
inline void checkFuse(const Frame& KF, uint64_t kfId, const std::vector<int32_t>& kfPoint, const MapPointTable& T,
                      const std::vector<int32_t>& queries, float th)
{
    const char* fn = "Fuse";
    checkDescriptors(KF, fn);
    const int n = T.size();
    if (!(th > 0.0f)) throw std::invalid_argument("Fuse: th must be positive");
    if (T.descriptors.size() != (size_t)n * 32) throw std::invalid_argument("Fuse: point descriptors are not n x 32 bytes");
    if (!T.bad.empty() && T.bad.size() != (size_t)n) throw std::invalid_argument("Fuse: bad flags are neither empty nor n entries long");
    if (T.obsStart.size() != (size_t)n + 1 || T.obsStart[0] != 0 || T.obsKf.size() < (size_t)std::max(T.obsStart.back(), 0))
        throw std::invalid_argument("Fuse: observation arrays of inconsistent lengths");
    for (int i = 0; i < n; i++) {
        if (T.obsStart[i + 1] < T.obsStart[i]) throw std::invalid_argument("Fuse: obsStart decreases");
        for (int k = T.obsStart[i] + 1; k < T.obsStart[i + 1]; k++)
            if (!(T.obsKf[k - 1] < T.obsKf[k])) throw std::invalid_argument("Fuse: an observation list is unsorted or repeats a key frame");
    }
    if (!kfPoint.empty() && kfPoint.size() != (size_t)KF.N()) throw std::invalid_argument("Fuse: kfPoint is neither empty nor N entries long");
    std::vector<uint8_t> seen(n, 0);
    for (int32_t o : kfPoint) {
        if (o < -1 || o >= n) throw std::invalid_argument("Fuse: a slot names a point outside the table");
        if (o < 0 || (!T.bad.empty() && T.bad[o])) continue;           // a bad occupant only makes its queries KF_POINT_BAD
        if (seen[o]) throw std::invalid_argument("Fuse: a point holds two slots of the key frame");
        seen[o] = 1;
        if (!std::binary_search(T.obsKf.begin() + T.obsStart[o], T.obsKf.begin() + T.obsStart[o + 1], kfId))
            throw std::invalid_argument("Fuse: the point in a slot does not list the key frame");
    }
    std::fill(seen.begin(), seen.end(), 0);
    for (int32_t q : queries) {
        if (q < -1 || q >= n) throw std::invalid_argument("Fuse: a query names a point outside the table");
        if (q < 0) continue;
        if (seen[q]) throw std::invalid_argument("Fuse: a map point is queried twice");
        seen[q] = 1;
    }
}
}  // namespace detail

class ORBmatcher {
 public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;     // ORBmatcher.cc:38-40
    ORBmatcher(pgorb_ctx* ctx, float nnratio = 0.6f, bool checkOri = true)
        : ctx_(ctx), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return pgorb_descriptor_distance(a, b); }
    // vbPrevMatched: 2 floats per F1 keypoint, updated in place; vnMatches12 resized to F1.N()
    int SearchForInitialization(Frame& F1, Frame& F2, std::vector<float>& vbPrevMatched,
                                std::vector<int32_t>& vnMatches12, int windowSize = 10)
    {
        // the library reads N descriptors of each frame and 2 * N1 floats of vbPrevMatched through these pointers
        detail::checkDescriptors(F1, "SearchForInitialization");
        detail::checkDescriptors(F2, "SearchForInitialization");
        if (vbPrevMatched.size() != (size_t)F1.N() * 2)
            throw std::invalid_argument("SearchForInitialization: vbPrevMatched does not hold 2 floats per F1 keypoint");
        vnMatches12.assign(F1.N(), -1);
        if (F1.N() == 0) return 0;
        const int rc = pgorb_search_for_initialization(ctx_, F1.mvKeysUndistorted.data(), F1.mDescriptors.data(), F1.N(),
                                                       F2.mvKeysUndistorted.data(), F2.mDescriptors.data(), F2.N(),
                                                       F2.mnMinX, F2.mnMaxX, F2.mnMinY, F2.mnMaxY,
                                                       vbPrevMatched.data(), vnMatches12.data(), windowSize, mfNNratio,
                                                       mbCheckOrientation ? 1 : 0);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        return rc;
    }
    // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo = false) (ORBmatcher.cc:659-825): F12 row-major
    // (F12.at<float>(r, c)), (ex, ey) the epipole in KF2 (:665-672), hasPoint[i] = GetMapPoint(i) != NULL (empty = none).
    int SearchForTriangulation(const Frame& KF1, const Frame& KF2, const FeatureVector& fv1, const FeatureVector& fv2,
                               const float F12[9], float ex, float ey, const std::vector<uint8_t>& hasPoint1,
                               const std::vector<uint8_t>& hasPoint2, std::vector<std::pair<size_t, size_t> >& vMatchedPairs)
    {
        // the library reads N mask entries, N descriptors and mStart[n] feature indices through these pointers
        detail::checkKeyFrame(KF1, fv1, hasPoint1, "SearchForTriangulation");
        detail::checkKeyFrame(KF2, fv2, hasPoint2, "SearchForTriangulation");
        vMatchedPairs.clear();
        std::vector<int32_t> m12(KF1.N() > 0 ? KF1.N() : 1, -1);
        const int rc = pgorb_search_for_triangulation(ctx_, KF1.mvKeysUndistorted.data(), KF1.mDescriptors.data(),
                                                      hasPoint1.empty() ? nullptr : hasPoint1.data(), KF1.N(),
                                                      fv1.mNode.data(), fv1.mStart.data(), fv1.mFeat.data(), fv1.size(),
                                                      KF2.mvKeysUndistorted.data(), KF2.mDescriptors.data(),
                                                      hasPoint2.empty() ? nullptr : hasPoint2.data(), KF2.N(),
                                                      fv2.mNode.data(), fv2.mStart.data(), fv2.mFeat.data(), fv2.size(),
                                                      F12, ex, ey, mbCheckOrientation ? 1 : 0, m12.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        vMatchedPairs.reserve(rc);
        for (int i = 0; i < KF1.N(); i++)                              // :814-822
            if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
        return rc;
    }

    // Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:827-979), monocular: KF's undistorted keypoints, descriptors and Frame bounds, its
    // pose and mnId; kfPoint[i] = the table index of GetMapPoint(i) or -1 (empty = all empty); queries[q] = the table index of
    // vpMapPoints[q] or -1 for NULL.  action[q] (PGORB_FUSE_*) says what the reference did with query q; the caller replays the
    // actions in query order (include/pgorb.h).  Returns nFused.
    int Fuse(const Frame& KF, const pgorb_kf_pose& pose, uint64_t kfId, const std::vector<int32_t>& kfPoint, const MapPointTable& table,
             const std::vector<int32_t>& queries, std::vector<int32_t>& action, float th = 3.0f, std::vector<int32_t>* bestIdx = nullptr,
             std::vector<int32_t>* bestDist = nullptr, std::vector<int32_t>* kfPointOut = nullptr)
    {
        detail::checkFuse(KF, kfId, kfPoint, table, queries, th);
        const int nq = (int)queries.size(), N = KF.N();
        action.assign(nq > 0 ? nq : 1, PGORB_FUSE_SKIPPED);
        std::vector<int32_t> bi(nq > 0 ? nq : 1, -1), bd(nq > 0 ? nq : 1, -1), out(N > 0 ? N : 1, -1);
        const int rc = pgorb_fuse(ctx_, KF.mvKeysUndistorted.data(), KF.mDescriptors.data(), N, &pose, kfId, KF.mnMinX, KF.mnMaxX,
                                  KF.mnMinY, KF.mnMaxY, kfPoint.empty() ? nullptr : kfPoint.data(), table.size(), table.points.data(),
                                  table.descriptors.data(), table.bad.empty() ? nullptr : table.bad.data(), table.obsStart.data(),
                                  table.obsKf.data(), nq, queries.data(), th, action.data(), bi.data(), bd.data(), out.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        action.resize(nq);
        if (bestIdx) bestIdx->assign(bi.begin(), bi.begin() + nq);
        if (bestDist) bestDist->assign(bd.begin(), bd.begin() + nq);
        if (kfPointOut) kfPointOut->assign(out.begin(), out.begin() + N);
        return rc;
    }

 private:
    pgorb_ctx* ctx_;
    float mfNNratio;
    bool mbCheckOrientation;
};

// The slice of ORB_SLAM2::KeyFrame that CreateNewMapPoints reads: mvKeysUn and mDescriptors, mFeatVec, which keypoints have a map
// point (empty = none), the pose and camera, and (for a neighbour) ComputeSceneMedianDepth(2).
struct KeyFrame {
    Frame frame;
    FeatureVector featVec;
    std::vector<uint8_t> hasPoint;
    pgorb_kf_pose pose{};
    float medianDepth = 0;
};

// The observation lists pgorb_refresh_map_points reads: point i observes key frame obsFrame[k] (a position in the call's key-frame
// list) at keypoint obsIdx[k] for k in obsStart[i] .. obsStart[i + 1], IN THE ORDER THE CALLER'S mObservations ITERATES
// (a std::map<KeyFrame*, size_t>: address order; include/pgorb.h); refObs[i] = the position of mpRefKF in point i's own list.
struct MapPointObservations {
    std::vector<int32_t> obsStart{0};
    std::vector<int32_t> obsFrame, obsIdx, refObs;
};

namespace detail {
// everything pgorb_refresh_map_points rejects, and the lengths it reads through its pointers
inline void checkRefresh(const std::vector<const KeyFrame*>& kfs, const std::vector<uint8_t>& kfBad, size_t npoints, size_t ndesc,
                         const std::vector<uint8_t>& pointBad, const MapPointObservations& O, const std::vector<int32_t>* select, int what);
}  // namespace detail

class CovisibilityGraph;

class LocalMapping {
 public:
    explicit LocalMapping(pgorb_ctx* ctx) : ctx_(ctx) {}
    // LocalMapping::MapPointCulling (LocalMapping.cc:170-207) over recent = mlpRecentAddedMapPoints as table indices; obsLive masks the
    // observation lists (include/pgorb.h).  kfPoint, pointBad (one flag per point) and obsLive are updated in place; action[t] =
    // PGORB_CULL_MP_*; survivors = the list afterwards.  Returns the number of points culled.  Defined below CovisibilityGraph.
    int MapPointCulling(std::vector<std::vector<int32_t>>& kfPoint, std::vector<uint8_t>& pointBad, const MapPointObservations& obs,
                        std::vector<uint8_t>& obsLive, const std::vector<int32_t>& firstKfId, const std::vector<int32_t>& visible,
                        const std::vector<int32_t>& found, const std::vector<int32_t>& recent, int curKfId, int thObs,
                        std::vector<int32_t>& action, std::vector<int32_t>& survivors, std::array<int32_t, PGORB_CULL_INFO>* info = nullptr);
    // LocalMapping::KeyFrameCulling (:634-698) with KeyFrame::SetBadFlag and MapPoint::EraseObservation over `graph` with
    // mpCurrentKeyFrame = curKf.  octaves[f][i] = mvKeysUn[i].octave; kfPoint, pointBad, obsLive, refObs, kfBad, kfToBeErased (one flag
    // per key frame) and the graph are updated in place; kfNotErase empty = none.  record = (key frame, nMPs, nRedundantObservations,
    // PGORB_CULL_KF_*) per list member; rowStatus [nkf] (PGORB_CULL_ROW_* bits).  Returns the number of key frames culled; info[0] ==
    // PGORB_CULL_LIMIT: the list is longer than listCap and nothing was done.
    int KeyFrameCulling(CovisibilityGraph& graph, int curKf, const std::vector<std::vector<int32_t>>& octaves,
                        std::vector<std::vector<int32_t>>& kfPoint, std::vector<uint8_t>& pointBad, const MapPointObservations& obs,
                        std::vector<uint8_t>& obsLive, std::vector<int32_t>& refObs, const std::vector<uint8_t>& kfNotErase,
                        std::vector<uint8_t>& kfBad, std::vector<uint8_t>& kfToBeErased, int listCap, std::vector<int32_t>& record,
                        std::vector<int32_t>& rowStatus, std::array<int32_t, PGORB_CULL_INFO>* info = nullptr);
    // MapPoint::AddObservation / Replace / EraseObservation with their KeyFrame slot writes (MapPoint.cc:119-232, KeyFrame.cc:313-336)
    // from an ordered edit list, with the result of applying the edits one after another (include/pgorb.h).  kfPoint, pointBad,
    // visible, found and replaced (one entry per point) are updated in place; obs with obs.refObs, masked by obsLive (empty = all
    // live), is read and obsOut (another object) receives the fresh lists and refObs; kfOrder empty = index order.  editStatus[e] =
    // PGORB_EDIT_* bits, touched[p] = PGORB_EDIT_TOUCH_* bits, selected = the points with touched & selectBits.  Returns the number
    // of edits applied; info[0] == PGORB_EDIT_LIMIT: a component is larger than PGORB_EDIT_MAX_BAG and nothing was done.
    int ApplyMapEdits(const std::vector<pgorb_map_edit>& edits, std::vector<std::vector<int32_t>>& kfPoint, const std::vector<int32_t>& kfOrder,
                      std::vector<uint8_t>& pointBad, std::vector<int32_t>& visible, std::vector<int32_t>& found, std::vector<int32_t>& replaced,
                      const MapPointObservations& obs, const std::vector<uint8_t>& obsLive, MapPointObservations& obsOut,
                      std::vector<int32_t>& editStatus, std::vector<int32_t>& touched, int selectBits, std::vector<int32_t>& selected,
                      std::array<int32_t, PGORB_EDIT_INFO>* info = nullptr)
    {
        const char* fn = "LocalMapping::ApplyMapEdits";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        const size_t np = pointBad.size(), nkf = kfPoint.size(), ne = edits.size();
        size_t real = 0;
        for (const pgorb_map_edit& e : edits) {
            if (e.op < PGORB_EDIT_NOP || e.op > PGORB_EDIT_SET_REF) fail("an unknown op");
            real += e.op != PGORB_EDIT_NOP;
        }
        if (ne > PGORB_EDIT_MAX_LIST || real > PGORB_EDIT_MAX_EDITS) fail("more than PGORB_EDIT_MAX_EDITS edits that are not NOP");
        if (visible.size() != np || found.size() != np || replaced.size() != np || obs.refObs.size() != np || obs.obsStart.size() != np + 1)
            fail("visible, found, replaced, refObs and obsStart need one entry per point");
        if (&obsOut == &obs) fail("obsOut aliases obs");
        if (!kfOrder.empty()) {
            if (kfOrder.size() != nkf) fail("kfOrder is not a permutation");
            std::vector<uint8_t> seen(nkf, 0);
            for (int32_t r : kfOrder) {
                if (r < 0 || r >= (int64_t)nkf || seen[r]) fail("kfOrder is not a permutation");
                seen[r] = 1;
            }
        }
        if (obs.obsStart[0] != 0) fail("obsStart must rise from 0");
        for (size_t p = 0; p < np; p++)
            if (obs.obsStart[p + 1] < obs.obsStart[p]) fail("obsStart must rise from 0");
        const size_t m = (size_t)obs.obsStart[np];
        if (obs.obsFrame.size() < m || obs.obsIdx.size() < m || (!obsLive.empty() && obsLive.size() < m)) fail("obsFrame, obsIdx and obsLive need one entry per observation");
        size_t live = 0, adds = 0;
        std::vector<int64_t> seenAt(nkf + 1, -1);
        for (size_t p = 0; p < np; p++) {
            const int len = obs.obsStart[p + 1] - obs.obsStart[p];
            if (len && (obs.refObs[p] < -1 || obs.refObs[p] >= len)) fail("refObs lies outside the point's list");
            for (int o = obs.obsStart[p]; o < obs.obsStart[p + 1]; o++) {
                if (!obsLive.empty() && !obsLive[o]) continue;
                const int f = obs.obsFrame[o];
                if (f < 0 || f >= (int64_t)nkf || obs.obsIdx[o] < 0 || obs.obsIdx[o] >= (int64_t)kfPoint[f].size()) fail("an observation names a key frame or keypoint out of range");
                if (seenAt[f] == (int64_t)p) fail("a list names a key frame twice");
                seenAt[f] = (int64_t)p;
                live++;
            }
        }
        for (const pgorb_map_edit& e : edits) adds += e.op == PGORB_EDIT_ADD;
        std::vector<int32_t*> slots(nkf + 1, nullptr);
        std::vector<int32_t> n(nkf + 1, 0);
        for (size_t f = 0; f < nkf; f++) { slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size(); }
        const size_t capOut = live + adds;
        obsOut.obsStart.assign(np + 1, 0);
        obsOut.obsFrame.assign(capOut + 1, 0); obsOut.obsIdx.assign(capOut + 1, 0); obsOut.refObs.assign(np + 1, -1);
        editStatus.assign(ne + 1, 0); touched.assign(np + 1, 0); selected.assign(np + 1, -1);
        std::array<int32_t, PGORB_EDIT_INFO> inf{};
        pgorb_map_edit none{};
        uint8_t one = 0;
        const int rc = pgorb_apply_map_edits(ctx_, ne ? edits.data() : &none, (int)ne, (int)nkf, slots.data(), n.data(), kfOrder.empty() ? nullptr : kfOrder.data(),
                                             (int)np, np ? pointBad.data() : &one, visible.data(), found.data(), replaced.data(), obs.obsStart.data(),
                                             obs.obsFrame.data(), obs.obsIdx.data(), obsLive.empty() ? nullptr : obsLive.data(), obs.refObs.data(), (int)capOut,
                                             obsOut.obsStart.data(), obsOut.obsFrame.data(), obsOut.obsIdx.data(), obsOut.refObs.data(), editStatus.data(),
                                             touched.data(), selectBits, (int)np, selected.data(), inf.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        const bool done = inf[0] != PGORB_EDIT_LIMIT;
        obsOut.obsFrame.resize(done ? (size_t)inf[1] : 0); obsOut.obsIdx.resize(done ? (size_t)inf[1] : 0); obsOut.refObs.resize(np);
        editStatus.resize(ne); touched.resize(np); selected.resize(done ? (size_t)inf[7] : 0);
        if (info) *info = inf;
        return rc;
    }
    // MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:259-324) and MapPoint::UpdateNormalAndDepth (:347-388) of many points in
    // one call, as LocalMapping.cc:444-446 and :519-532 run them.  keyFrames: frame (mvKeysUn, mDescriptors) and pose are read;
    // kfBad[f] = isBad() (empty = none); points / descriptors (32 bytes each) / pointBad (empty = none) are the table, refreshed
    // in place; select = table indices (NULL = all); what = PGORB_MP_DESCRIPTOR | PGORB_MP_NORMAL_DEPTH | PGORB_MP_BOTH.
    // status[q] / bestObs[q] per selected point (include/pgorb.h).  Returns the number of points with a positive status.
    int RefreshMapPoints(const std::vector<const KeyFrame*>& keyFrames, const std::vector<uint8_t>& kfBad,
                         std::vector<pgorb_map_point>& points, std::vector<uint8_t>& descriptors, const std::vector<uint8_t>& pointBad,
                         const MapPointObservations& obs, const std::vector<int32_t>* select, int what, std::vector<int32_t>& status,
                         std::vector<int32_t>* bestObs = nullptr)
    {
        detail::checkRefresh(keyFrames, kfBad, points.size(), descriptors.size(), pointBad, obs, select, what);
        const size_t nkf = keyFrames.size(), np = points.size();
        std::vector<const pgorb_keypoint*> kps(nkf + 1);
        std::vector<const uint8_t*> desc(nkf + 1);
        std::vector<int32_t> n(nkf + 1);
        std::vector<pgorb_kf_pose> pose(nkf + 1);
        for (size_t f = 0; f < nkf; f++) {
            kps[f] = keyFrames[f]->frame.mvKeysUndistorted.data(); desc[f] = keyFrames[f]->frame.mDescriptors.data();
            n[f] = keyFrames[f]->frame.N(); pose[f] = keyFrames[f]->pose;
        }
        const int nsel = select ? (int)select->size() : (int)np;
        status.assign(nsel > 0 ? nsel : 1, 0);
        std::vector<int32_t> best(nsel > 0 ? nsel : 1, -1);
        const int rc = pgorb_refresh_map_points(ctx_, (int)nkf, kps.data(), desc.data(), n.data(), pose.data(),
                                                kfBad.empty() ? nullptr : kfBad.data(), (int)np, points.data(), descriptors.data(),
                                                pointBad.empty() ? nullptr : pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(),
                                                obs.obsIdx.data(), obs.refObs.empty() ? nullptr : obs.refObs.data(), nsel,
                                                select ? (nsel ? select->data() : best.data()) : nullptr, what, best.data(), status.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        status.resize(nsel);
        if (bestObs) bestObs->assign(best.begin(), best.begin() + nsel);
        return rc;
    }
    // CreateNewMapPoints() (LocalMapping.cc:209-454), monocular: neighbours in GetBestCovisibilityKeyFrames order.  points in
    // the reference's creation order, count[s] per neighbour (PGORB_CNM_SKIPPED: the baseline test skipped it), hasPoint1Out KF1's
    // mask afterwards.  The map bookkeeping is the caller's (include/pgorb.h).  Returns the number of points.
    int CreateNewMapPoints(const KeyFrame& KF1, const std::vector<const KeyFrame*>& neighbours, std::vector<pgorb_new_map_point>& points,
                           std::vector<int32_t>& count, std::vector<uint8_t>* hasPoint1Out = nullptr)
    {
        const size_t nn = neighbours.size();
        if (nn > PGORB_CNM_MAX_NEIGHBOURS) throw std::invalid_argument("CreateNewMapPoints: more than 64 neighbours");
        detail::checkKeyFrame(KF1.frame, KF1.featVec, KF1.hasPoint, "CreateNewMapPoints");
        std::vector<const pgorb_keypoint*> kps(nn + 1);
        std::vector<const uint8_t*> desc(nn + 1), has(nn + 1);
        std::vector<const uint32_t*> node(nn + 1), feat(nn + 1);
        std::vector<const int32_t*> start(nn + 1);
        std::vector<int32_t> n(nn + 1), nfv(nn + 1);
        std::vector<pgorb_kf_pose> pose(nn + 1);
        std::vector<float> median(nn + 1);
        for (size_t s = 0; s < nn; s++) {
            if (!neighbours[s]) throw std::invalid_argument("CreateNewMapPoints: a neighbour is NULL");
            const KeyFrame& K = *neighbours[s];
            detail::checkKeyFrame(K.frame, K.featVec, K.hasPoint, "CreateNewMapPoints");
            kps[s] = K.frame.mvKeysUndistorted.data(); desc[s] = K.frame.mDescriptors.data();
            has[s] = K.hasPoint.empty() ? nullptr : K.hasPoint.data();
            node[s] = K.featVec.mNode.data(); start[s] = K.featVec.mStart.data(); feat[s] = K.featVec.mFeat.data();
            n[s] = K.frame.N(); nfv[s] = K.featVec.size(); pose[s] = K.pose; median[s] = K.medianDepth;
        }
        const int n1 = KF1.frame.N();
        points.resize(n1 > 0 ? n1 : 1);
        count.assign(nn > 0 ? nn : 1, 0);
        std::vector<uint8_t> hout(n1 > 0 ? n1 : 1);
        const int rc = pgorb_create_new_map_points(ctx_, KF1.frame.mvKeysUndistorted.data(), KF1.frame.mDescriptors.data(),
                                                   KF1.hasPoint.empty() ? nullptr : KF1.hasPoint.data(), n1, KF1.featVec.mNode.data(),
                                                   KF1.featVec.mStart.data(), KF1.featVec.mFeat.data(), KF1.featVec.size(), &KF1.pose,
                                                   (int)nn, kps.data(), desc.data(), has.data(), n.data(), node.data(), start.data(),
                                                   feat.data(), nfv.data(), pose.data(), median.data(), points.data(), count.data(),
                                                   nullptr, nullptr, hout.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        points.resize(rc);
        count.resize(nn);
        if (hasPoint1Out) hasPoint1Out->assign(hout.begin(), hout.begin() + n1);
        return rc;
    }

 private:
    pgorb_ctx* ctx_;
};

// What Optimizer::PoseOptimization returns beside the pose (include/pgorb.h).
struct PoseOptimizationResult {
    int inliers = 0;                       // the reference's return value
    pgorb_kf_pose pose{};                  // a complete record: Tcw, Ow, the input's camera
    std::vector<uint8_t> outlier;          // mvbOutlier
    std::vector<int32_t> kpPoint;          // the slots afterwards (discardOutliers empties the outliers')
    std::vector<float> chi2;
    int nmatchesMap = 0;
    int32_t info[PGORB_PO_INFO] = {};      // status, rounds, iterations of rounds 0..3, trials, edges
};

// What Optimizer::OptimizeSim3 returns beside nIn (include/pgorb.h).
struct OptimizeSim3Result {
    int inliers = 0;                       // nIn, the reference's return value
    pgorb_sim3_estimate estimate{};        // R12, t12, s12 of the recovered g2o::Sim3 (the input with a status)
    std::vector<int32_t> matches12;        // the merged input with every removed correspondence set to -1
    std::vector<float> chi2_12, chi2_21;
    pgorb_kf_pose scwPose{};               // gScm*gSmw decomposed, with KF1's camera: what SearchByProjection(pKF, Scw, ...) takes
    int32_t info[PGORB_OS3_INFO] = {};     // status, nCorrespondences, nBad, iterations and trials of both optimize calls, nMoreIterations
};

// What Optimizer::LocalBundleAdjustment returns beside the number of erased observations (include/pgorb.h).
struct LocalBundleAdjustmentResult {
    int erased = 0;                        // vToErase.size(), the library's return value
    std::vector<pgorb_kf_pose> poses;      // per key frame: the local ones adjusted (complete records), the others as given
    std::vector<uint8_t> erase, level;     // per observation, aligned with the lists
    std::vector<float> chi2;
    std::vector<std::pair<int32_t, int32_t>> toErase;   // vToErase as (key frame, point), in list order
    std::vector<uint8_t> isLocal, role;    // per point; per key frame: PGORB_LBA_ROLE_*
    int32_t info[PGORB_LBA_INFO] = {};     // status, edges, local points, local and fixed key frames, iterations and trials of both optimize calls, level-1 edges
};

// The essential graph as the caller's containers hold it (include/pgorb.h, pgorb_optimize_essential_graph): key frames by index in
// strictly rising mnId order; every list holds candidates, the library applies the filters.
struct EssentialGraph {
    std::vector<uint64_t> kfId;                       // mnId
    std::vector<pgorb_kf_pose> pose;
    std::vector<uint8_t> kfBad;                       // empty = none
    int loopKf = 0, curKf = 0;
    std::vector<uint8_t> hasCorrected, hasNonCorrected;      // empty = an empty map
    std::vector<pgorb_sim3d> corrected, nonCorrected;        // CorrectedSim3, NonCorrectedSim3
    std::vector<int32_t> loopConn;                    // (i, j, weight) triples in LoopConnections' iteration order
    std::vector<int32_t> parent;                      // GetParent() or -1
    std::vector<int32_t> loopEdgeStart, loopEdge;     // GetLoopEdges() per key frame, CSR
    std::vector<int32_t> covisStart, covis, covisWeight;     // the covisibles per key frame with weights, CSR
    std::vector<int32_t> pointRefKf;                  // per point: the key frame Optimizer.cc:1020-1029 selects, or -1
};

// What Optimizer::OptimizeEssentialGraph returns beside the number of optimised vertices.
struct EssentialGraphResult {
    int optimised = 0;
    std::vector<pgorb_sim3d> sim3;         // the recovered estimates (zeros for a bad key frame)
    std::vector<pgorb_kf_pose> poses;      // [R | t/s] with Ow for a key frame with an edge, the input for the others
    std::vector<pgorb_eg_edge> edges;      // the derived edges (vertex 0, vertex 1, kind) with their final chi2
    int32_t info[PGORB_EG_INFO] = {};      // status, vertices, free vertices, edges per kind, iterations, trials, envelope blocks
};

// What Optimizer::GlobalBundleAdjustment returns beside the number of free active vertices (include/pgorb.h).
struct GlobalBundleAdjustmentResult {
    int optimised = 0;
    std::vector<pgorb_kf_pose> poses;      // per key frame: every one that is not bad replaced (complete records), a bad one as given
    std::vector<float> pos;                // [npoints][3]: the included points adjusted, the others as given
    std::vector<uint8_t> kfDone, pointDone;      // what mnBAGlobalForKF = nLoopKF marks
    std::vector<float> chi2;               // per observation, aligned with the lists
    int32_t info[PGORB_GBA_INFO] = {};     // status, edges, included points, vertices, free active vertices, iterations, trials, envelope blocks
};

class Optimizer {
 public:
    explicit Optimizer(pgorb_ctx* ctx) : ctx_(ctx) {}
    // Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag, nLoopKF, bRobust) (Optimizer.cc:41-237), monocular, on the GPU.
    // keyFrames IN RISING mnId ORDER: frame (mvKeysUn: pt and octave) and pose are read; kfBad[f] = isBad(), kfFixedId0[f] = (mnId == 0)
    // (empty = none).  points (pos is read; with inPlace, the nLoopKF == 0 branch, replaced for the done points), pointBad (empty =
    // none) and obs are the table.  nIterations: 10 from loop closing, 20 from initialisation; bRobust: Huber with (float)sqrt(5.99).
    // Everything pgorb_global_bundle_adjustment refuses as a bad argument is a std::invalid_argument here, before the library is
    // called; a map past a capacity is the library's error (std::runtime_error).
    GlobalBundleAdjustmentResult GlobalBundleAdjustment(const std::vector<const KeyFrame*>& keyFrames, const std::vector<uint8_t>& kfBad,
                                                        const std::vector<uint8_t>& kfFixedId0, std::vector<pgorb_map_point>& points,
                                                        const std::vector<uint8_t>& pointBad, const MapPointObservations& obs,
                                                        int nIterations = 10, bool bRobust = false, bool inPlace = false)
    {
        const auto fail = [](const char* m) { throw std::invalid_argument(std::string("GlobalBundleAdjustment: ") + m); };
        const size_t nkf = keyFrames.size(), np = points.size();
        const int levels = pgorb_levels(ctx_);
        if (nIterations < 0) fail("nIterations is negative");
        if ((!kfBad.empty() && kfBad.size() != nkf) || (!kfFixedId0.empty() && kfFixedId0.size() != nkf)) fail("kfBad or kfFixedId0 is neither empty nor one entry per key frame");
        if (!pointBad.empty() && pointBad.size() != np) fail("pointBad is neither empty nor one entry per point");
        std::vector<const pgorb_keypoint*> kps(nkf + 1);
        std::vector<int32_t> n(nkf + 1);
        std::vector<pgorb_kf_pose> pose(nkf + 1);
        for (size_t f = 0; f < nkf; f++) {
            if (!keyFrames[f]) fail("a key frame is NULL");
            const Frame& F = keyFrames[f]->frame;
            const pgorb_kf_pose& P = keyFrames[f]->pose;
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(P.Tcw[k])) fail("a pose is not finite");
            if (!std::isfinite(P.fx) || !std::isfinite(P.fy) || !std::isfinite(P.cx) || !std::isfinite(P.cy)) fail("a camera is not finite");
            if (P.fx == 0.0f || P.fy == 0.0f) fail("fx or fy is zero");
            if (F.N() > 16000) fail("more than 16000 keypoints in a key frame");
            kps[f] = F.mvKeysUndistorted.data(); n[f] = F.N(); pose[f] = P;
        }
        for (const pgorb_map_point& p : points)
            if (!std::isfinite(p.pos[0]) || !std::isfinite(p.pos[1]) || !std::isfinite(p.pos[2])) fail("a point is not finite");
        if (obs.obsStart.size() != np + 1 || obs.obsStart[0] != 0) fail("obsStart is not npoints + 1 entries rising from 0");
        for (size_t p = 0; p < np; p++) if (obs.obsStart[p + 1] < obs.obsStart[p]) fail("obsStart decreases");
        const size_t nobs = (size_t)obs.obsStart[np];
        if (obs.obsFrame.size() < nobs || obs.obsIdx.size() < nobs) fail("obsFrame or obsIdx is shorter than obsStart says");
        std::vector<int32_t> seen(nkf + 1, -1);
        for (size_t p = 0; p < np; p++)
            for (int k = obs.obsStart[p]; k < obs.obsStart[p + 1]; k++) {
                const int f = obs.obsFrame[k], i = obs.obsIdx[k];
                if (f < 0 || f >= (int)nkf || i < 0 || i >= n[f]) fail("an observation names a key frame or keypoint out of range");
                if (seen[f] == (int)p) fail("a list names a key frame twice");
                seen[f] = (int)p;
                const int o = kps[f][i].octave;
                if (levels > 0 && (o < 0 || o >= levels)) fail("an octave is outside the context's levels");
            }
        GlobalBundleAdjustmentResult r;
        r.poses.resize(nkf + 1);
        r.pos.assign(3 * (np + 1), 0.0f); r.kfDone.assign(nkf + 1, 0); r.pointDone.assign(np + 1, 0); r.chi2.assign(nobs + 1, 0.0f);
        std::vector<pgorb_map_point> none(1);
        const int rc = pgorb_global_bundle_adjustment(ctx_, (int)nkf, kps.data(), n.data(), pose.data(), kfBad.empty() ? nullptr : kfBad.data(),
                                                      kfFixedId0.empty() ? nullptr : kfFixedId0.data(), (int)np, np ? points.data() : none.data(),
                                                      pointBad.empty() ? nullptr : pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(),
                                                      obs.obsIdx.data(), nIterations, bRobust ? 1 : 0, inPlace ? 1 : 0, r.poses.data(), r.pos.data(),
                                                      r.kfDone.data(), r.pointDone.data(), r.chi2.data(), r.info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.poses.resize(nkf); r.pos.resize(3 * np); r.kfDone.resize(nkf); r.pointDone.resize(np); r.chi2.resize(nobs);
        r.optimised = rc;
        return r;
    }
    // Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
    // (Optimizer.cc:781-1044) on the GPU.  points (pos is read and corrected in place) and pointBad (empty = none) are the table;
    // pMP->UpdateNormalAndDepth() is pgorb_refresh_map_points with PGORB_MP_NORMAL_DEPTH afterwards.  Everything
    // pgorb_optimize_essential_graph refuses as a bad argument is a std::invalid_argument here, before the library is called, and so is
    // an empty key-frame list (the library answers that one with PGORB_EG_NOTHING); a graph past a capacity is the library's error
    // (std::runtime_error).
    EssentialGraphResult OptimizeEssentialGraph(const EssentialGraph& g, std::vector<pgorb_map_point>& points, const std::vector<uint8_t>& pointBad,
                                                bool bFixScale = false, int minFeat = 100, int iterations = 20)
    {
        const auto fail = [](const char* m) { throw std::invalid_argument(std::string("OptimizeEssentialGraph: ") + m); };
        const size_t nkf = g.kfId.size(), np = points.size();
        const auto simOk = [](const pgorb_sim3d& S) {
            for (double v : S.r) if (!std::isfinite(v)) return false;
            for (double v : S.t) if (!std::isfinite(v)) return false;
            return std::isfinite(S.s) && S.s > 0.0;
        };
        if (iterations < 0) fail("iterations is negative");
        if (!nkf) fail("no key frame");
        if (g.pose.size() != nkf || g.parent.size() != nkf) fail("pose or parent is not one entry per key frame");
        if (!g.kfBad.empty() && g.kfBad.size() != nkf) fail("kfBad is neither empty nor one entry per key frame");
        if (!pointBad.empty() && pointBad.size() != np) fail("pointBad is neither empty nor one entry per point");
        if (g.pointRefKf.size() != np) fail("pointRefKf is not one entry per point");
        if (g.loopKf < 0 || g.loopKf >= (int)nkf || g.curKf < 0 || g.curKf >= (int)nkf) fail("loopKf or curKf is out of range");
        if ((!g.hasCorrected.empty() && (g.hasCorrected.size() != nkf || g.corrected.size() != nkf)) ||
            (!g.hasNonCorrected.empty() && (g.hasNonCorrected.size() != nkf || g.nonCorrected.size() != nkf))) fail("a Sim3 map is not one entry per key frame");
        for (size_t i = 0; i < nkf; i++) {
            if (i && !(g.kfId[i] > g.kfId[i - 1])) fail("kfId is not strictly rising");
            if (g.parent[i] < -1 || g.parent[i] >= (int)nkf || g.parent[i] == (int)i) fail("a parent is out of range");
            for (int k = 0; k < 12; k++) if (!std::isfinite(g.pose[i].Tcw[k])) fail("a pose is not finite");
            if ((!g.hasCorrected.empty() && g.hasCorrected[i] && !simOk(g.corrected[i])) ||
                (!g.hasNonCorrected.empty() && g.hasNonCorrected[i] && !simOk(g.nonCorrected[i]))) fail("a Sim3 is not finite or its scale is not positive");
        }
        if (g.loopConn.size() % 3) fail("loopConn is not a list of triples");
        for (size_t k = 0; k + 2 < g.loopConn.size(); k += 3)
            if (g.loopConn[k] < 0 || g.loopConn[k] >= (int)nkf || g.loopConn[k + 1] < 0 || g.loopConn[k + 1] >= (int)nkf || g.loopConn[k] == g.loopConn[k + 1])
                fail("a loop connection is out of range or joins a key frame to itself");
        const auto rows = [&](const std::vector<int32_t>& start, const std::vector<int32_t>& val, const char* what) {
            if (start.size() != nkf + 1 || start[0] != 0) fail(what);
            for (size_t i = 0; i < nkf; i++) {
                if (start[i + 1] < start[i] || (size_t)start[i + 1] > val.size()) fail(what);
                for (int k = start[i]; k < start[i + 1]; k++) if (val[k] < 0 || val[k] >= (int)nkf || val[k] == (int)i) fail(what);
            }
        };
        rows(g.loopEdgeStart, g.loopEdge, "the loop edges are not a CSR of key frames");
        rows(g.covisStart, g.covis, "the covisibles are not a CSR of key frames");
        if (g.covisWeight.size() < g.covis.size()) fail("covisWeight is shorter than covis");
        for (size_t p = 0; p < np; p++) {
            if (g.pointRefKf[p] < -1 || g.pointRefKf[p] >= (int)nkf) fail("pointRefKf is out of range");
            if (!std::isfinite(points[p].pos[0]) || !std::isfinite(points[p].pos[1]) || !std::isfinite(points[p].pos[2])) fail("a point is not finite");
        }
        const size_t ncand = g.loopConn.size() / 3 + nkf + (size_t)g.loopEdgeStart[nkf] + (size_t)g.covisStart[nkf];
        EssentialGraphResult r;
        r.sim3.resize(nkf); r.poses.resize(nkf); r.edges.resize(ncand + 1);
        std::vector<pgorb_map_point> none(1);
        std::vector<int32_t> one(1, 0);
        const int rc = pgorb_optimize_essential_graph(ctx_, (int)nkf, g.kfId.data(), g.pose.data(), g.kfBad.empty() ? nullptr : g.kfBad.data(),
                                                      g.loopKf, g.curKf, bFixScale ? 1 : 0, g.hasCorrected.empty() ? nullptr : g.hasCorrected.data(),
                                                      g.corrected.data(), g.hasNonCorrected.empty() ? nullptr : g.hasNonCorrected.data(),
                                                      g.nonCorrected.data(), (int)(g.loopConn.size() / 3), g.loopConn.empty() ? one.data() : g.loopConn.data(),
                                                      g.parent.data(), g.loopEdgeStart.data(), g.loopEdge.empty() ? one.data() : g.loopEdge.data(),
                                                      g.covisStart.data(), g.covis.empty() ? one.data() : g.covis.data(),
                                                      g.covisWeight.empty() ? one.data() : g.covisWeight.data(), minFeat, iterations, (int)np,
                                                      np ? points.data() : none.data(), pointBad.empty() ? nullptr : pointBad.data(),
                                                      np ? g.pointRefKf.data() : one.data(), r.sim3.data(), r.poses.data(), r.edges.data(), r.info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.edges.resize((size_t)(r.info[3] + r.info[4] + r.info[5] + r.info[6]));
        r.optimised = rc;
        return r;
    }
    // Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) (Optimizer.cc:453-778), monocular, on the GPU.  keyFrames: frame
    // (mvKeysUn: pt and octave) and pose are read; kfBad[f] = isBad(), kfFixedId0[f] = (mnId == 0) (empty = none); kfPoint[f][i] = the
    // table index of GetMapPoint(i) or -1; localKf: pKF and its covisible key frames as positions in keyFrames.  points (pos is read
    // and, for the local points, replaced in place), pointBad (empty = none) and obs (obsStart / obsFrame / obsIdx) are the table.
    // rounds: 2, or 1 for bDoMore == false.  Everything pgorb_local_bundle_adjustment refuses as a bad argument is a
    // std::invalid_argument here, before the library is called; a window past a capacity is the library's error (std::runtime_error).
    LocalBundleAdjustmentResult LocalBundleAdjustment(const std::vector<const KeyFrame*>& keyFrames, const std::vector<uint8_t>& kfBad,
                                                      const std::vector<uint8_t>& kfFixedId0, const std::vector<std::vector<int32_t>>& kfPoint,
                                                      const std::vector<int32_t>& localKf, std::vector<pgorb_map_point>& points,
                                                      const std::vector<uint8_t>& pointBad, const MapPointObservations& obs, int rounds = 2)
    {
        const auto fail = [](const char* m) { throw std::invalid_argument(std::string("LocalBundleAdjustment: ") + m); };
        const size_t nkf = keyFrames.size(), np = points.size();
        const int levels = pgorb_levels(ctx_);
        if (rounds < 1 || rounds > 2) fail("rounds is neither 1 nor 2");
        if (kfPoint.size() != nkf) fail("kfPoint is not one list per key frame");
        if ((!kfBad.empty() && kfBad.size() != nkf) || (!kfFixedId0.empty() && kfFixedId0.size() != nkf)) fail("kfBad or kfFixedId0 is neither empty nor one entry per key frame");
        if (!pointBad.empty() && pointBad.size() != np) fail("pointBad is neither empty nor one entry per point");
        std::vector<const pgorb_keypoint*> kps(nkf + 1);
        std::vector<const int32_t*> slots(nkf + 1);
        std::vector<int32_t> n(nkf + 1);
        std::vector<pgorb_kf_pose> pose(nkf + 1);
        for (size_t f = 0; f < nkf; f++) {
            if (!keyFrames[f]) fail("a key frame is NULL");
            const Frame& F = keyFrames[f]->frame;
            const pgorb_kf_pose& P = keyFrames[f]->pose;
            if (kfPoint[f].size() != (size_t)F.N()) fail("a key frame's slots are not N entries long");
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(P.Tcw[k])) fail("a pose is not finite");
            if (!std::isfinite(P.fx) || !std::isfinite(P.fy) || !std::isfinite(P.cx) || !std::isfinite(P.cy)) fail("a camera is not finite");
            if (P.fx == 0.0f || P.fy == 0.0f) fail("fx or fy is zero");
            for (int s : kfPoint[f]) if (s < -1 || s >= (int)np) fail("a slot names a point outside the table");
            if (F.N() > 16000) fail("more than 16000 keypoints in a key frame");
            kps[f] = F.mvKeysUndistorted.data(); slots[f] = kfPoint[f].data(); n[f] = F.N(); pose[f] = P;
        }
        for (int f : localKf) if (f < 0 || f >= (int)nkf) fail("a local key frame is out of range");
        for (const pgorb_map_point& p : points)
            if (!std::isfinite(p.pos[0]) || !std::isfinite(p.pos[1]) || !std::isfinite(p.pos[2])) fail("a point is not finite");
        if (obs.obsStart.size() != np + 1 || obs.obsStart[0] != 0) fail("obsStart is not npoints + 1 entries rising from 0");
        for (size_t p = 0; p < np; p++) if (obs.obsStart[p + 1] < obs.obsStart[p]) fail("obsStart decreases");
        const size_t nobs = (size_t)obs.obsStart[np];
        if (obs.obsFrame.size() < nobs || obs.obsIdx.size() < nobs) fail("obsFrame or obsIdx is shorter than obsStart says");
        std::vector<int32_t> seen(nkf + 1, -1);
        for (size_t p = 0; p < np; p++)
            for (int k = obs.obsStart[p]; k < obs.obsStart[p + 1]; k++) {
                const int f = obs.obsFrame[k], i = obs.obsIdx[k];
                if (f < 0 || f >= (int)nkf || i < 0 || i >= n[f]) fail("an observation names a key frame or keypoint out of range");
                if (seen[f] == (int)p) fail("a list names a key frame twice");
                seen[f] = (int)p;
                const int o = kps[f][i].octave;
                if (levels > 0 && (o < 0 || o >= levels)) fail("an octave is outside the context's levels");
            }
        LocalBundleAdjustmentResult r;
        r.poses.resize(nkf + 1);
        r.erase.assign(nobs + 1, 0); r.level.assign(nobs + 1, 0); r.chi2.assign(nobs + 1, 0.0f);
        r.isLocal.assign(np + 1, 0); r.role.assign(nkf + 1, 0);
        std::vector<pgorb_map_point> none(1);
        const int rc = pgorb_local_bundle_adjustment(ctx_, (int)nkf, kps.data(), n.data(), pose.data(), kfBad.empty() ? nullptr : kfBad.data(),
                                                     slots.data(), kfFixedId0.empty() ? nullptr : kfFixedId0.data(), (int)localKf.size(),
                                                     localKf.data(), (int)np, np ? points.data() : none.data(),
                                                     pointBad.empty() ? nullptr : pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(),
                                                     obs.obsIdx.data(), rounds, r.poses.data(), r.erase.data(), r.chi2.data(), r.level.data(),
                                                     r.isLocal.data(), r.role.data(), r.info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.poses.resize(nkf); r.erase.resize(nobs); r.level.resize(nobs); r.chi2.resize(nobs); r.isLocal.resize(np); r.role.resize(nkf);
        for (size_t p = 0; p < np; p++)
            for (int k = obs.obsStart[p]; k < obs.obsStart[p + 1]; k++)
                if (r.erase[k]) r.toErase.emplace_back(obs.obsFrame[k], (int32_t)p);
        r.erased = rc;
        return r;
    }
    // Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:1046-1241) on the GPU.  The key frames, the
    // slots and the table as for Sim3Solver; matches12[i1]: the KF2 keypoint or -1 (the solver's matches12Out); newMatches12 (empty =
    // none): what SearchBySim3 wrote, replacing an entry where it is >= 0; estimate: the solver's `found`.
    // Everything pgorb_optimize_sim3 refuses is a std::invalid_argument here, before the library is called.
    OptimizeSim3Result OptimizeSim3(const Frame& F1, const Frame& F2, const pgorb_kf_pose& pose1, const pgorb_kf_pose& pose2,
                                    const std::vector<int32_t>& kfPoint1, const std::vector<int32_t>& kfPoint2,
                                    const std::vector<int32_t>& matches12, const std::vector<int32_t>& newMatches12,
                                    const std::vector<pgorb_map_point>& points, const std::vector<uint8_t>& pointBad,
                                    const pgorb_sim3_estimate& estimate, float th2 = 10.0f, bool bFixScale = false)
    {
        const auto fail = [](const char* m) { throw std::invalid_argument(std::string("OptimizeSim3: ") + m); };
        const int n1 = F1.N(), n2 = F2.N(), np = (int)points.size(), levels = pgorb_levels(ctx_);
        if (kfPoint1.size() != (size_t)n1 || matches12.size() != (size_t)n1) fail("kfPoint1 or matches12 is not N1 entries long");
        if (!newMatches12.empty() && newMatches12.size() != (size_t)n1) fail("newMatches12 is neither empty nor N1 entries long");
        if (kfPoint2.size() != (size_t)n2) fail("kfPoint2 is not N2 entries long");
        if (!pointBad.empty() && pointBad.size() != (size_t)np) fail("pointBad is neither empty nor one entry per point");
        for (const pgorb_kf_pose* P : {&pose1, &pose2}) {
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(P->Tcw[k])) fail("a pose is not finite");
            if (!std::isfinite(P->fx) || !std::isfinite(P->fy) || !std::isfinite(P->cx) || !std::isfinite(P->cy)) fail("a camera is not finite");
        }
        for (int k = 0; k < 9; k++) if (!std::isfinite(estimate.R12[k])) fail("the estimate is not finite");
        for (int k = 0; k < 3; k++) if (!std::isfinite(estimate.t12[k])) fail("the estimate is not finite");
        if (!std::isfinite(estimate.s12)) fail("the estimate is not finite");
        if (!(estimate.s12 > 0.0f)) fail("the estimate's scale is not positive");
        if (!(th2 > 0.0f) || !std::isfinite(th2)) fail("th2 is not positive");
        for (int s : kfPoint1) if (s < -1 || s >= np) fail("a slot names a point outside the table");
        for (int s : kfPoint2) if (s < -1 || s >= np) fail("a slot names a point outside the table");
        for (int i = 0; i < n1; i++) {
            if (matches12[i] < -1 || matches12[i] >= n2) fail("matches12 is outside [-1, n2)");
            if (!newMatches12.empty() && (newMatches12[i] < -1 || newMatches12[i] >= n2)) fail("newMatches12 is outside [-1, n2)");
            const int j = (!newMatches12.empty() && newMatches12[i] >= 0) ? newMatches12[i] : matches12[i];
            if (j < 0 || kfPoint1[i] < 0 || kfPoint2[j] < 0) continue;
            const int o1 = F1.mvKeysUndistorted[i].octave, o2 = F2.mvKeysUndistorted[j].octave;
            if (levels > 0 && (o1 < 0 || o1 >= levels || o2 < 0 || o2 >= levels)) fail("an octave is outside the context's levels");
            for (const float* p : {points[kfPoint1[i]].pos, points[kfPoint2[j]].pos})
                if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) fail("a referenced point is not finite");
        }
        if (n1 > 16000 || n2 > 16000) fail("more than 16000 keypoints in a key frame");
        OptimizeSim3Result r;
        r.matches12.assign(n1 > 0 ? n1 : 1, -1); r.chi2_12.assign(n1 > 0 ? n1 : 1, 0.0f); r.chi2_21.assign(n1 > 0 ? n1 : 1, 0.0f);
        const int rc = pgorb_optimize_sim3(ctx_, F1.mvKeysUndistorted.data(), n1, &pose1, kfPoint1.data(), F2.mvKeysUndistorted.data(), n2, &pose2,
                                           kfPoint2.data(), matches12.data(), newMatches12.empty() ? nullptr : newMatches12.data(), np, points.data(),
                                           pointBad.empty() ? nullptr : pointBad.data(), &estimate, th2, bFixScale ? 1 : 0, &r.estimate,
                                           r.matches12.data(), r.chi2_12.data(), r.chi2_21.data(), &r.scwPose, r.info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.matches12.resize(n1); r.chi2_12.resize(n1); r.chi2_21.resize(n1);
        r.inliers = rc;
        return r;
    }
    // Optimizer::PoseOptimization(pFrame) (Optimizer.cc:239-451), monocular, on the GPU.  F: mvKeysUn (pt and octave are read); pose:
    // the frame's pose and camera; kpPoint[i] = the table index of mvpMapPoints[i] or -1; points: the table (pos is read);
    // pointHasObs: Observations() > 0 per point (empty = all).  discardOutliers: the loop of Tracking.cc:768-787 runs too.
    // Everything pgorb_pose_optimization refuses is a std::invalid_argument here, before the library is called.
    PoseOptimizationResult PoseOptimization(const Frame& F, const pgorb_kf_pose& pose, const std::vector<int32_t>& kpPoint,
                                            const std::vector<pgorb_map_point>& points, const std::vector<uint8_t>& pointHasObs,
                                            bool discardOutliers = false)
    {
        const auto fail = [](const char* m) { throw std::invalid_argument(std::string("PoseOptimization: ") + m); };
        const int n = F.N(), np = (int)points.size(), levels = pgorb_levels(ctx_);
        if (kpPoint.size() != (size_t)n) fail("kpPoint is not N entries long");
        if (!pointHasObs.empty() && pointHasObs.size() != (size_t)np) fail("pointHasObs is neither empty nor one entry per point");
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(pose.Tcw[k])) fail("the pose is not finite");
        if (!std::isfinite(pose.fx) || !std::isfinite(pose.fy) || !std::isfinite(pose.cx) || !std::isfinite(pose.cy)) fail("the camera is not finite");
        if (pose.fx == 0.0f || pose.fy == 0.0f) fail("fx or fy is zero");
        for (int i = 0; i < n; i++) {
            const int s = kpPoint[i];
            if (s < -1 || s >= np) fail("a slot names a point outside the table");
            if (s < 0) continue;
            const int o = F.mvKeysUndistorted[i].octave;
            if (levels > 0 && (o < 0 || o >= levels)) fail("an octave is outside the context's levels");      // (no context: the library's error)
            if (!std::isfinite(points[s].pos[0]) || !std::isfinite(points[s].pos[1]) || !std::isfinite(points[s].pos[2])) fail("a referenced point is not finite");
        }
        PoseOptimizationResult r;
        r.outlier.assign(n > 0 ? n : 1, 0); r.kpPoint.assign(n > 0 ? n : 1, -1); r.chi2.assign(n > 0 ? n : 1, 0.0f);
        const int rc = pgorb_pose_optimization(ctx_, F.mvKeysUndistorted.data(), n, &pose, kpPoint.data(), np, points.data(),
                                               pointHasObs.empty() ? nullptr : pointHasObs.data(), discardOutliers ? 1 : 0, &r.pose, r.outlier.data(),
                                               r.kpPoint.data(), &r.nmatchesMap, r.chi2.data(), r.info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.outlier.resize(n); r.kpPoint.resize(n); r.chi2.resize(n);
        r.inliers = rc;
        return r;
    }
 private:
    pgorb_ctx* ctx_;
};

// Sim3Solver (src/Sim3Solver.cc) on the GPU, with the reference's surface.  mnIterations and mnBestInliers live here and go to the
// library as first_iteration / best_inliers_in, so iterate(5) can be called again on the same solver (LoopClosing.cc:274-342).
// F1, F2: mvKeysUn (the octave is read); pose1, pose2: Tcw and each key frame's own camera; kfPoint1 / kfPoint2: the table index of
// every slot's point or -1 (the caller owns GetIndexInKeyFrame); matches12[i1]: the KF2 keypoint SearchByBoW matched, or -1; points
// (pos is read) and pointBad (empty = none) the table; draws: [>= maxIterations][3] raw rand() values in [0, 2^31), 3 per iteration.
// Everything pgorb_sim3_solver refuses is a std::invalid_argument here, before the library is called.
class Sim3Solver {
 public:
    Sim3Solver(pgorb_ctx* ctx, const Frame& F1, const Frame& F2, const pgorb_kf_pose& pose1, const pgorb_kf_pose& pose2,
               const std::vector<int32_t>& kfPoint1, const std::vector<int32_t>& kfPoint2, const std::vector<int32_t>& matches12,
               const std::vector<pgorb_map_point>& points, const std::vector<uint8_t>& pointBad, std::vector<uint32_t> draws,
               bool bFixScale = false)
        : ctx_(ctx), F1_(F1), F2_(F2), pose1_(pose1), pose2_(pose2), kfPoint1_(kfPoint1), kfPoint2_(kfPoint2), matches12_(matches12),
          points_(points), pointBad_(pointBad), draws_(std::move(draws)), mbFixScale(bFixScale)
    {
        const int n1 = F1.N(), n2 = F2.N(), np = (int)points.size(), levels = pgorb_levels(ctx_);
        if (kfPoint1.size() != (size_t)n1 || matches12.size() != (size_t)n1) fail("kfPoint1 or matches12 is not N1 entries long");
        if (kfPoint2.size() != (size_t)n2) fail("kfPoint2 is not N2 entries long");
        if (!pointBad.empty() && pointBad.size() != (size_t)np) fail("pointBad is neither empty nor one entry per point");
        for (const pgorb_kf_pose* P : {&pose1, &pose2}) {
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(P->Tcw[k])) fail("a pose is not finite");
            if (!std::isfinite(P->fx) || !std::isfinite(P->fy) || !std::isfinite(P->cx) || !std::isfinite(P->cy)) fail("a camera is not finite");
        }
        for (int s : kfPoint1) if (s < -1 || s >= np) fail("a slot names a point outside the table");
        for (int s : kfPoint2) if (s < -1 || s >= np) fail("a slot names a point outside the table");
        for (int i = 0; i < n1; i++) {
            const int j = matches12[i];
            if (j < -1 || j >= n2) fail("matches12 is outside [-1, n2)");
            if (j < 0 || kfPoint1[i] < 0 || kfPoint2[j] < 0) continue;
            const int o1 = F1.mvKeysUndistorted[i].octave, o2 = F2.mvKeysUndistorted[j].octave;
            if (levels > 0 && (o1 < 0 || o1 >= levels || o2 < 0 || o2 >= levels)) fail("an octave is outside the context's levels");
            for (const float* p : {points[kfPoint1[i]].pos, points[kfPoint2[j]].pos})
                if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) fail("a referenced point is not finite");
        }
        if (n1 > 16000 || n2 > 16000) fail("more than 16000 keypoints in a key frame");
        SetRansacParameters();
    }
    // Sim3Solver.cc:114-138; resets mnIterations as the reference does (mnBestInliers stays)
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        if (minInliers < 3) fail("minInliers is below 3");
        if (!((float)probability > 0.0f && (float)probability < 1.0f)) fail("probability is outside (0, 1)");
        if (maxIterations < 1) fail("maxIterations is below 1");
        if (maxIterations > PGORB_SIM3_MAX_ITERATIONS) fail("maxIterations above PGORB_SIM3_MAX_ITERATIONS");
        if (draws_.size() < (size_t)maxIterations * 3) fail("fewer than maxIterations x 3 draws");
        for (size_t k = 0; k < (size_t)maxIterations * 3; k++)
            if (draws_[k] >= 0x80000000u) fail("a draw is not below 2^31");
        mRansacProb = probability; mRansacMinInliers = minInliers; mRansacMaxIts = maxIterations;
        mnIterations = 0;
    }
    // Sim3Solver::iterate (:140-207): true = a hypothesis was returned; T12 = [s*R | t] row-major 4 x 4
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float T12[16] = nullptr)
    {
        if (nIterations < 1) fail("nIterations is below 1");
        if (mnIterations < 0) fail("mnIterations is negative");
        const int n1 = F1_.N(), n2 = F2_.N();
        pgorb_sim3_params prm{(float)mRansacProb, mRansacMinInliers, mRansacMaxIts, mbFixScale ? 1 : 0, mnIterations, nIterations, mnBestInliers};
        std::vector<uint8_t> fl(n1 > 0 ? n1 : 1, 0);
        matches12Out.assign(n1 > 0 ? n1 : 1, -1); already1.assign(n1 > 0 ? n1 : 1, 0); already2.assign(n2 > 0 ? n2 : 1, 0);
        pgorb_sim3_estimate b{};
        const int rc = pgorb_sim3_solver(ctx_, F1_.mvKeysUndistorted.data(), n1, &pose1_, kfPoint1_.data(), F2_.mvKeysUndistorted.data(), n2,
                                         &pose2_, kfPoint2_.data(), matches12_.data(), (int)points_.size(), points_.data(),
                                         pointBad_.empty() ? nullptr : pointBad_.data(), &prm, draws_.data(), &found, &foundSim3, &b, fl.data(),
                                         matches12Out.data(), already1.data(), already2.data(), info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        matches12Out.resize(n1); already1.resize(n1); already2.resize(n2);
        mnIterations = info[3]; mnBestInliers = info[5];
        if (info[6] >= 0) best = b;
        bNoMore = (info[0] & (PGORB_S3_FEW | PGORB_S3_NO_MORE)) != 0;
        vbInliers.assign(n1, false);
        for (int i = 0; i < n1; i++) vbInliers[i] = fl[i] != 0;
        nInliers = rc;
        const bool ok = (info[0] & PGORB_S3_FOUND) != 0;
        if (ok && T12) {
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T12[4 * r + c] = foundSim3.sR12[3 * r + c]; T12[4 * r + 3] = foundSim3.t12[r]; }
            T12[12] = T12[13] = T12[14] = 0.0f; T12[15] = 1.0f;
        }
        return ok;
    }
    bool find(std::vector<bool>& vbInliers12, int& nInliers, float T12[16] = nullptr)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
    }
    const float* GetEstimatedRotation() const { return best.R12; }         // 3 x 3 row-major
    const float* GetEstimatedTranslation() const { return best.t12; }
    float GetEstimatedScale() const { return best.s12; }

    int mnIterations = 0, mnBestInliers = 0;
    pgorb_sim3_estimate found{}, best{};
    pgorb_sim3 foundSim3{};                                                 // what pgorb_search_by_sim3 takes
    std::vector<int32_t> matches12Out;                                      // LoopClosing.cc:313-318
    std::vector<uint8_t> already1, already2;                                // ORBmatcher.cc:1133-1146
    int32_t info[PGORB_S3_INFO] = {};
 private:
    static void fail(const char* m) { throw std::invalid_argument(std::string("Sim3Solver: ") + m); }
    pgorb_ctx* ctx_;
    const Frame& F1_; const Frame& F2_;
    pgorb_kf_pose pose1_, pose2_;
    std::vector<int32_t> kfPoint1_, kfPoint2_, matches12_;
    std::vector<pgorb_map_point> points_;
    std::vector<uint8_t> pointBad_;
    std::vector<uint32_t> draws_;
    bool mbFixScale;
    double mRansacProb = 0.99; int mRansacMinInliers = 6, mRansacMaxIts = 300;
};

// PnPsolver (thirdparty/orb-slam2/src/PnPsolver.cc) with the reference's surface: the constructor, SetRansacParameters, iterate(n)
// and find.  mnIterations, mnBestInliers, mvbBestInliers (by keypoint) and mBestTcw live here and go to the library with every call, so
// iterate(5) can be called again on the same solver as Tracking::Relocalization does.  F: the lost frame (mvKeysUndistorted: pt and
// octave are read); camera: fx, fy, cx, cy are read; kpPoint: the table index of vpMapPointMatches[i] or -1; points (pos is read) and
// pointBad (empty = none) the table; draws: [>= max(maxIterations, nIterations)][4] raw rand() values in [0, 2^31).
// Everything pgorb_pnp_solver refuses is a std::invalid_argument here, before the library is called.
class PnPsolver {
 public:
    PnPsolver(pgorb_ctx* ctx, const Frame& F, const pgorb_kf_pose& camera, const std::vector<int32_t>& kpPoint,
              const std::vector<pgorb_map_point>& points, const std::vector<uint8_t>& pointBad, std::vector<uint32_t> draws)
        : ctx_(ctx), n_(F.N()), keys_(F.mvKeysUndistorted), camera_(camera), kpPoint_(kpPoint), points_(points), pointBad_(pointBad), draws_(std::move(draws))
    {
        const int n = F.N(), np = (int)points.size(), levels = pgorb_levels(ctx_);
        if (kpPoint.size() != (size_t)n) fail("kpPoint is not N entries long");
        if (!pointBad.empty() && pointBad.size() != (size_t)np) fail("pointBad is neither empty nor one entry per point");
        if (!std::isfinite(camera.fx) || !std::isfinite(camera.fy) || !std::isfinite(camera.cx) || !std::isfinite(camera.cy)) fail("the camera is not finite");
        for (int i = 0; i < n; i++) {
            const int s = kpPoint[i];
            if (s < -1 || s >= np) fail("a slot names a point outside the table");
            if (s < 0 || (!pointBad.empty() && pointBad[s])) continue;
            const pgorb_keypoint& k = F.mvKeysUndistorted[i];
            if (levels > 0 && (k.octave < 0 || k.octave >= levels)) fail("an octave is outside the context's levels");
            const float* p = points[s].pos;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(k.x) || !std::isfinite(k.y))
                fail("a referenced point or keypoint is not finite");
            N_++;
        }
        if (n > 16000) fail("more than 16000 keypoints in the frame");
        mvbBestInliers.assign(n > 0 ? n : 1, 0);
        SetRansacParameters();
    }
    // PnPsolver.cc:121-157 (the header's defaults); the adjusted minimum and the cap come from pgorb_pnp_ransac
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                             float th2 = 5.991f)
    {
        prm_ = pgorb_pnp_params{(float)probability, minInliers, maxIterations, minSet, epsilon, th2, 0, 1, 0};
        checkParams(prm_);
        int32_t mi = 0, cap = 0;
        pgorb_pnp_ransac(prm_.probability, minInliers, maxIterations, minSet, epsilon, N_, &mi, &cap);
        mRansacMinInliers = mi; mRansacMaxIts = cap;
    }
    // PnPsolver::iterate (:165-258): true = a pose was returned; Tcw = the 4 x 4 float pose, row-major
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tcw[16] = nullptr)
    {
        pgorb_pnp_params prm = prm_;
        prm.first_iteration = mnIterations; prm.niterations = nIterations; prm.best_inliers_in = mnBestInliers;
        checkParams(prm);
        const int n = n_;
        const size_t W = (size_t)std::max(prm.max_iterations, prm.niterations);
        if (draws_.size() < W * 4) fail("fewer than max(maxIterations, nIterations) x 4 draws");
        for (size_t k = 0; k < W * 4; k++)
            if (draws_[k] >= 0x80000000u) fail("a draw is not below 2^31");
        std::vector<uint8_t> fl(n > 0 ? n : 1, 0), bi(n > 0 ? n : 1, 0);
        kpPointOut.assign(n > 0 ? n : 1, -1);
        pgorb_kf_pose bp{};
        const int rc = pgorb_pnp_solver(ctx_, keys_.data(), n, &camera_, kpPoint_.data(), (int)points_.size(), points_.data(),
                                        pointBad_.empty() ? nullptr : pointBad_.data(), &prm, draws_.data(), mvbBestInliers.data(), &mBestTcw,
                                        &pose, fl.data(), kpPointOut.data(), bi.data(), &bp, nullptr, info);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        kpPointOut.resize(n);
        mnIterations = info[4]; mnBestInliers = info[6];
        mvbBestInliers = bi; mBestTcw = bp;
        bNoMore = (info[0] & PGORB_PNP_NO_MORE) != 0;
        vbInliers.assign(n, false);
        for (int i = 0; i < n; i++) vbInliers[i] = fl[i] != 0;
        nInliers = rc;
        const bool ok = (info[0] & PGORB_PNP_FOUND) != 0;
        if (ok && Tcw) {
            for (int k = 0; k < 12; k++) Tcw[k] = pose.Tcw[k];
            Tcw[12] = Tcw[13] = Tcw[14] = 0.0f; Tcw[15] = 1.0f;
        }
        return ok;
    }
    bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16] = nullptr)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers, Tcw);
    }

    int mnIterations = 0, mnBestInliers = 0, mRansacMinInliers = 0, mRansacMaxIts = 0;
    std::vector<uint8_t> mvbBestInliers;                                    // by keypoint
    pgorb_kf_pose mBestTcw{};
    pgorb_kf_pose pose{};                                                   // what pgorb_pose_optimization takes (Tracking.cc:1405)
    std::vector<int32_t> kpPointOut;                                        // Tracking.cc:1411-1420: no point where vbInliers is false
    int32_t info[PGORB_PNP_INFO] = {};
 private:
    static void fail(const char* m) { throw std::invalid_argument(std::string("PnPsolver: ") + m); }
    static void checkParams(const pgorb_pnp_params& p)
    {
        if (p.min_set != 4) fail("minSet must be 4");
        if (p.min_inliers < 1) fail("minInliers is below 1");
        if (!(p.probability > 0.0f && p.probability < 1.0f)) fail("probability is outside (0, 1)");
        if (!(p.epsilon > 0.0f && p.epsilon <= 1.0f)) fail("epsilon is outside (0, 1]");
        if (!(p.th2 > 0.0f)) fail("th2 is not positive");
        if (p.max_iterations < 1 || p.niterations < 1 || p.first_iteration < 0) fail("maxIterations or nIterations below 1, or a negative first iteration");
        if (std::max(p.max_iterations, p.niterations) > PGORB_PNP_MAX_WINDOW) fail("a window above PGORB_PNP_MAX_WINDOW");
    }
    pgorb_ctx* ctx_;
    int n_;
    std::vector<pgorb_keypoint> keys_;                                      // a copy, as every other input: the solver may outlive its Frame
    pgorb_kf_pose camera_;
    std::vector<int32_t> kpPoint_;
    std::vector<pgorb_map_point> points_;
    std::vector<uint8_t> pointBad_;
    std::vector<uint32_t> draws_;
    pgorb_pnp_params prm_{};
    int N_ = 0;
};

// Initializer (src/Initializer.cc) over pgorb_initializer: the constructor and Initialize.  ReferenceFrame / CurrentFrame:
// mvKeysUndistorted (pt is read); camera: fx, fy, cx, cy are read (mK); draws: [>= iterations][8] raw rand() values in [0, 2^31).
// After Initialize: pose (Tracking.cc:622-626), matches12Out (Tracking.cc:612-619) and the map of CreateInitialMapMonocular
// (points, kfPoint1, kfPoint2, obs) as pgorb_refresh_map_points and pgorb_global_bundle_adjustment read it.
// Everything pgorb_initializer refuses is a std::invalid_argument here, before the library is called.
class Initializer {
 public:
    Initializer(pgorb_ctx* ctx, const Frame& ReferenceFrame, const pgorb_kf_pose& camera, std::vector<uint32_t> draws, float sigma = 1.0f,
                int iterations = 200, float minParallax = 1.0f, int minTriangulated = 50)
        : ctx_(ctx), keys1_(ReferenceFrame.mvKeysUndistorted), camera_(camera), draws_(std::move(draws)),
          prm_{sigma, iterations, minParallax, minTriangulated}
    {
        keys1_.resize(ReferenceFrame.N());
        checkKeys(keys1_);
        if (!std::isfinite(camera.fx) || !std::isfinite(camera.fy) || !std::isfinite(camera.cx) || !std::isfinite(camera.cy)) fail("the camera is not finite");
        if (!(sigma > 0.0f) || !std::isfinite(sigma) || !std::isfinite(minParallax)) fail("sigma must be positive and finite, minParallax finite");
        if (iterations < 1) fail("iterations is below 1");
        if (iterations > PGORB_INIT_MAX_ITERATIONS) fail("iterations above PGORB_INIT_MAX_ITERATIONS");
        if (draws_.size() < (size_t)iterations * 8) fail("fewer than iterations x 8 draws");
        for (size_t k = 0; k < (size_t)iterations * 8; k++)
            if (draws_[k] >= 0x80000000u) fail("a draw is not below 2^31");
    }
    // Initializer::Initialize (:44-121): R21 [9] and t21 [3] row-major (written when true), vP3D [n1][3], vbTriangulated [n1]
    bool Initialize(const Frame& CurrentFrame, const std::vector<int32_t>& vMatches12, float R21[9], float t21[3],
                    std::vector<std::array<float, 3>>& vP3D, std::vector<bool>& vbTriangulated)
    {
        std::vector<pgorb_keypoint> keys2(CurrentFrame.mvKeysUndistorted);
        keys2.resize(CurrentFrame.N());
        checkKeys(keys2);
        const int n1 = (int)keys1_.size(), n2 = (int)keys2.size();
        if (vMatches12.size() != (size_t)n1) fail("vMatches12 is not N entries long");
        for (int i = 0; i < n1; i++)
            if (vMatches12[i] < -1 || vMatches12[i] >= n2) fail("vMatches12 is outside [-1, n2)");
        const size_t c1 = n1 > 0 ? n1 : 1, c2 = n2 > 0 ? n2 : 1;
        std::vector<float> p3d(3 * c1, 0.0f);
        std::vector<uint8_t> tri(c1, 0);
        matches12Out.assign(c1, -1);
        points.assign(c1, pgorb_map_point{});
        kfPoint1.assign(c1, -1); kfPoint2.assign(c2, -1);
        obsStart.assign(c1 + 1, 0); obsFrame.assign(2 * c1, -1); obsIdx.assign(2 * c1, -1);
        int32_t np = 0;
        const int rc = pgorb_initializer(ctx_, keys1_.data(), n1, keys2.data(), n2, &camera_, vMatches12.data(), &prm_, draws_.data(), pose,
                                         p3d.data(), tri.data(), matches12Out.data(), points.data(), kfPoint1.data(), kfPoint2.data(),
                                         obsStart.data(), obsFrame.data(), obsIdx.data(), &np, nullptr, info, finfo);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        matches12Out.resize(n1); kfPoint1.resize(n1); kfPoint2.resize(n2);
        points.resize(np); obsStart.resize(np + 1); obsFrame.resize(2 * np); obsIdx.resize(2 * np);
        vP3D.assign(n1, std::array<float, 3>{});
        vbTriangulated.assign(n1, false);
        for (int i = 0; i < n1; i++) { vP3D[i] = {p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]}; vbTriangulated[i] = tri[i] != 0; }
        const bool ok = (info[0] & PGORB_INIT_OK) != 0;
        if (ok)
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R21[3 * r + c] = pose[1].Tcw[4 * r + c]; t21[r] = pose[1].Tcw[4 * r + 3]; }
        return ok;
    }

    pgorb_kf_pose pose[2] = {};                                             // the reference frame's identity pose, [R21 | t21]
    std::vector<int32_t> matches12Out, kfPoint1, kfPoint2, obsStart, obsFrame, obsIdx;
    std::vector<pgorb_map_point> points;
    int32_t info[PGORB_INIT_INFO] = {};
    float finfo[PGORB_INIT_FINFO] = {};
 private:
    static void fail(const char* m) { throw std::invalid_argument(std::string("Initializer: ") + m); }
    static void checkKeys(const std::vector<pgorb_keypoint>& k)
    {
        if (k.size() > 16000) fail("more than 16000 keypoints in the frame");
        for (const pgorb_keypoint& q : k)
            if (!std::isfinite(q.x) || !std::isfinite(q.y)) fail("a keypoint coordinate is not finite");
    }
    pgorb_ctx* ctx_;
    std::vector<pgorb_keypoint> keys1_;                                     // a copy: the initializer may outlive its Frame
    pgorb_kf_pose camera_;
    std::vector<uint32_t> draws_;
    pgorb_init_params prm_;
};

namespace detail {
inline void checkRefresh(const std::vector<const KeyFrame*>& kfs, const std::vector<uint8_t>& kfBad, size_t npoints, size_t ndesc,
                         const std::vector<uint8_t>& pointBad, const MapPointObservations& O, const std::vector<int32_t>* select, int what)
{
    const char* fn = "RefreshMapPoints";
    const auto fail = [&](const char* m) { throw std::invalid_argument(std::string(fn) + ": " + m); };
    if (what < PGORB_MP_DESCRIPTOR || what > PGORB_MP_BOTH) fail("what is not PGORB_MP_DESCRIPTOR, PGORB_MP_NORMAL_DEPTH or PGORB_MP_BOTH");
    const int nkf = (int)kfs.size(), np = (int)npoints;
    for (const KeyFrame* K : kfs) {
        if (!K) fail("a key frame is NULL");
        checkDescriptors(K->frame, fn);
    }
    if (!kfBad.empty() && kfBad.size() != kfs.size()) fail("kfBad is neither empty nor one entry per key frame");
    if (ndesc != npoints * 32) fail("point descriptors are not n x 32 bytes");
    if (!pointBad.empty() && pointBad.size() != npoints) fail("pointBad is neither empty nor n entries long");
    if (O.obsStart.size() != npoints + 1 || O.obsStart[0] != 0) fail("obsStart is not n + 1 entries from 0");
    for (int i = 0; i < np; i++) if (O.obsStart[i + 1] < O.obsStart[i]) fail("obsStart decreases");
    const int m = O.obsStart[np];
    if (O.obsFrame.size() < (size_t)m || O.obsIdx.size() < (size_t)m) fail("fewer observations than obsStart says");
    for (int k = 0; k < m; k++)
        if (O.obsFrame[k] < 0 || O.obsFrame[k] >= nkf || O.obsIdx[k] < 0 || O.obsIdx[k] >= kfs[O.obsFrame[k]]->frame.N())
            fail("an observation names a key frame or keypoint out of range");
    std::vector<int32_t> seen(nkf > 0 ? nkf : 1, -1);
    for (int i = 0; i < np; i++)
        for (int k = O.obsStart[i]; k < O.obsStart[i + 1]; k++) {
            if (seen[O.obsFrame[k]] == i) fail("a list names a key frame twice");
            seen[O.obsFrame[k]] = i;
        }
    if ((what & PGORB_MP_NORMAL_DEPTH) && O.refObs.size() != npoints) fail("refObs is not n entries long");
    if (!(what & PGORB_MP_NORMAL_DEPTH) && !O.refObs.empty() && O.refObs.size() != npoints) fail("refObs is neither empty nor n entries long");
    std::vector<uint8_t> chosen(np > 0 ? np : 1, 0);
    const int nsel = select ? (int)select->size() : np;
    for (int q = 0; q < nsel; q++) {
        const int p = select ? (*select)[q] : q;
        if (p < 0 || p >= np) fail("a selection index is out of range");
        if (chosen[p]) fail("a point is selected twice");
        chosen[p] = 1;
        const int len = O.obsStart[p + 1] - O.obsStart[p];
        if ((what & PGORB_MP_NORMAL_DEPTH) && !(!pointBad.empty() && pointBad[p]) && len > 0 && len <= PGORB_MP_MAX_OBS &&
            (O.refObs[p] < 0 || O.refObs[p] >= len))
            fail("refObs lies outside the point's list");
    }
}

// what pgorb_update_connections and pgorb_update_local_map both reject of the slots, the observation lists and the ranks
inline void checkCovisTable(const char* fn, size_t nkf, const std::vector<std::vector<int32_t>>& kfPoint, size_t npoints,
                            const std::vector<uint8_t>& pointBad, const MapPointObservations& O, const std::vector<int32_t>& kfOrder)
{
    auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
    if (kfPoint.size() != nkf) fail("one slot array per key frame");
    if (nkf > PGORB_COVIS_MAX_KF) fail("more than PGORB_COVIS_MAX_KF key frames");
    for (const auto& s : kfPoint) {
        if (s.size() > 16000) fail("more than 16000 keypoints");
        for (int32_t p : s) if (p < -1 || p >= (int64_t)npoints) fail("a slot names a point out of range");
    }
    if (!pointBad.empty() && pointBad.size() != npoints) fail("pointBad needs one flag per point");
    if (O.obsStart.size() != npoints + 1 || O.obsStart[0] != 0) fail("obsStart needs npoints + 1 entries rising from 0");
    for (size_t i = 0; i < npoints; i++) if (O.obsStart[i + 1] < O.obsStart[i]) fail("obsStart decreases");
    if ((int64_t)O.obsFrame.size() < O.obsStart[npoints]) fail("obsFrame is shorter than obsStart says");
    std::vector<int32_t> seen(nkf + 1, -1);
    for (size_t i = 0; i < npoints; i++)
        for (int k = O.obsStart[i]; k < O.obsStart[i + 1]; k++) {
            const int f = O.obsFrame[k];
            if (f < 0 || f >= (int64_t)nkf) fail("an observation names a key frame out of range");
            if (seen[f] == (int32_t)i) fail("a list names a key frame twice");
            seen[f] = (int32_t)i;
        }
    if (!kfOrder.empty()) {
        if (kfOrder.size() != nkf) fail("kfOrder needs one rank per key frame");
        std::vector<uint8_t> used(nkf + 1, 0);
        for (int32_t r : kfOrder) {
            if (r < 0 || r >= (int64_t)nkf || used[r]) fail("kfOrder is not a permutation");
            used[r] = 1;
        }
    }
}
}  // namespace detail

// The covisibility graph of nkf key frames as the arrays the library keeps (include/pgorb.h): connKf / connW / nconn =
// mConnectedKeyFrameWeights in address order, ordKf / ordW / nord = mvpOrderedConnectedKeyFrames / mvOrderedWeights, parent
// (-1 = none) and firstConnection.  kfOrder[f] = the rank of key frame f's address (empty = index order); kfId0[f] = mnId == 0.
class CovisibilityGraph {
 public:
    CovisibilityGraph(pgorb_ctx* ctx, int nkf, int connCap, std::vector<int32_t> kfOrder = {}, std::vector<uint8_t> kfId0 = {})
        : ctx_(ctx), nkf_(nkf), connCap_(connCap), kfOrder(std::move(kfOrder)), kfId0(std::move(kfId0))
    {
        if (nkf < 0 || nkf > PGORB_COVIS_MAX_KF) throw std::invalid_argument("CovisibilityGraph: nkf outside 0..PGORB_COVIS_MAX_KF");
        if (connCap < 1 || connCap > PGORB_COVIS_MAX_CONN) throw std::invalid_argument("CovisibilityGraph: connCap outside 1..PGORB_COVIS_MAX_CONN");
        const size_t k1 = (size_t)std::max(nkf, 1);
        connKf.assign(k1 * connCap, -1); connW.assign(k1 * connCap, 0); ordKf.assign(k1 * connCap, -1); ordW.assign(k1 * connCap, 0);
        nconn.assign(k1, 0); nord.assign(k1, 0); parent.assign(k1, -1); firstConnection.assign(k1, 1);
    }
    int nkf() const { return nkf_; }
    int connCap() const { return connCap_; }
    // KeyFrame::UpdateConnections() (KeyFrame.cc:392-482) of `keyFrames` one after another, in place.  kfPoint[f] = the table
    // indices of key frame f's slots (-1 = none).  rowStatus [nkf] (PGORB_COVIS_* bits); loopConn (when loopConnCap > 0) =
    // LoopConnections (LoopClosing.cc:548-566) as (i, j, weight) records.  Returns the number of rows rewritten from their counters.
    int UpdateConnections(const std::vector<std::vector<int32_t>>& kfPoint, size_t npoints, const std::vector<uint8_t>& pointBad,
                          const MapPointObservations& obs, const std::vector<int32_t>& keyFrames, int th, std::vector<int32_t>& rowStatus,
                          int loopConnCap = 0, std::vector<std::array<int32_t, 3>>* loopConn = nullptr, std::array<int32_t, PGORB_COVIS_INFO>* info = nullptr)
    {
        const char* fn = "CovisibilityGraph::UpdateConnections";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        detail::checkCovisTable(fn, (size_t)nkf_, kfPoint, npoints, pointBad, obs, kfOrder);
        if (th < 1 || loopConnCap < 0) fail("th < 1 or loopConnCap < 0");
        if (!kfId0.empty() && kfId0.size() != (size_t)nkf_) fail("kfId0 needs one flag per key frame");
        std::vector<uint8_t> listed((size_t)nkf_ + 1, 0);
        for (int32_t f : keyFrames) {
            if (f < 0 || f >= nkf_) fail("a list entry is out of range");
            if (listed[f]) fail("the list names a key frame twice");
            listed[f] = 1;
        }
        checkRows(fn);
        std::vector<const int32_t*> slots((size_t)nkf_ + 1, nullptr);
        std::vector<int32_t> n((size_t)nkf_ + 1, 0);
        for (int f = 0; f < nkf_; f++) { slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size(); }
        rowStatus.assign((size_t)std::max(nkf_, 1), 0);
        std::vector<int32_t> loop((size_t)std::max(loopConnCap, 1) * 3, 0);
        std::array<int32_t, PGORB_COVIS_INFO> inf{};
        const int rc = pgorb_update_connections(ctx_, nkf_, slots.data(), n.data(), (int)npoints, pointBad.empty() ? nullptr : pointBad.data(),
                                                obs.obsStart.data(), obs.obsFrame.data(), kfOrder.empty() ? nullptr : kfOrder.data(),
                                                kfId0.empty() ? nullptr : kfId0.data(), (int)keyFrames.size(), keyFrames.empty() ? n.data() : keyFrames.data(),
                                                th, connCap_, connKf.data(), connW.data(), nconn.data(), ordKf.data(), ordW.data(), nord.data(),
                                                parent.data(), firstConnection.data(), rowStatus.data(), loopConnCap, loopConnCap ? loop.data() : nullptr,
                                                inf.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        rowStatus.resize((size_t)nkf_);
        if (info) *info = inf;
        if (loopConn) {
            loopConn->clear();
            const int m = (inf[0] & PGORB_COVIS_LIMIT) ? 0 : std::min(inf[1], loopConnCap);
            for (int e = 0; e < m; e++) loopConn->push_back({loop[3 * e], loop[3 * e + 1], loop[3 * e + 2]});
        }
        return rc;
    }
    // what pgorb_update_connections and pgorb_keyframe_culling reject of the rows: the counts, the address order of the map, the
    // ordered entries inside it, the parents
    void checkRows(const char* fn) const
    {
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        std::vector<int32_t> mark((size_t)nkf_ + 1, -1);
        for (int f = 0; f < nkf_; f++) {
            if (nconn[f] < 0 || nconn[f] > connCap_ || nord[f] < 0 || nord[f] > connCap_) fail("a row count is outside [0, connCap]");
            if (parent[f] < -1 || parent[f] >= nkf_) fail("a parent is out of range");
            int last = -1;
            for (int t = 0; t < nconn[f]; t++) {
                const int j = connKf[(size_t)f * connCap_ + t];
                if (j < 0 || j >= nkf_ || j == f) fail("a connection is out of range");
                const int r = kfOrder.empty() ? j : kfOrder[j];
                if (r <= last) fail("a connection row is not in address order");
                last = r; mark[j] = f;
            }
            for (int t = 0; t < nord[f]; t++) {
                const int j = ordKf[(size_t)f * connCap_ + t];
                if (j < 0 || j >= nkf_ || mark[j] != f) fail("an ordered entry is not in the row's map");
            }
        }
    }
    // GetBestCovisibilityKeyFrames(N) (KeyFrame.cc:277-285)
    std::vector<int32_t> GetBestCovisibilityKeyFrames(int f, int N) const
    {
        const int32_t* row = &ordKf[(size_t)f * connCap_];
        return std::vector<int32_t>(row, row + std::min((int)nord[f], std::max(N, 0)));
    }
    // GetCovisiblesByWeight(w) (:287-302): upper_bound with weightComp; when no weight is below w the reference returns an empty vector
    std::vector<int32_t> GetCovisiblesByWeight(int f, int w) const
    {
        const int32_t* row = &ordKf[(size_t)f * connCap_];
        int len = 0;
        for (int t = 0; t < nord[f]; t++) len += ordW[(size_t)f * connCap_ + t] >= w;
        return std::vector<int32_t>(row, row + (len == nord[f] ? 0 : len));
    }
    std::vector<int32_t> connKf, connW, nconn, ordKf, ordW, nord, parent;
    std::vector<uint8_t> firstConnection;
 private:
    pgorb_ctx* ctx_;
    int nkf_, connCap_;
 public:
    std::vector<int32_t> kfOrder;
    std::vector<uint8_t> kfId0;
};

struct LocalMapResult {
    std::vector<int32_t> kpPoint, localKf, queries;   // the frame's slots after the first loop, mvpLocalKeyFrames, mvpLocalMapPoints
    int refKf = -1, status = 0;                        // -1: mpReferenceKF is kept; PGORB_LOCALMAP_* bits
};

class Tracking {
 public:
    explicit Tracking(pgorb_ctx* ctx) : ctx_(ctx) {}
    // Tracking::UpdateLocalMap (Tracking.cc:1186-1321) for a frame whose mvpMapPoints are the table indices kpPoint (-1 = none), over
    // `graph` and the key frames' slots; prevLocalKf = mvpLocalKeyFrames before the call (NULL = none), walked again when no point votes.
    LocalMapResult UpdateLocalMap(const CovisibilityGraph& graph, const std::vector<int32_t>& kpPoint, const std::vector<std::vector<int32_t>>& kfPoint,
                                  size_t npoints, const std::vector<uint8_t>& pointBad, const MapPointObservations& obs, const std::vector<uint8_t>& kfBad,
                                  const std::vector<int32_t>* prevLocalKf = nullptr, int nbest = 10, int maxLocal = 80, int lkfCap = 256, int qcap = 16000)
    {
        const char* fn = "Tracking::UpdateLocalMap";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        const int nkf = graph.nkf(), cc = graph.connCap();
        if (nkf + 1 > PGORB_COVIS_MAX_KF) fail("more than PGORB_COVIS_MAX_KF - 1 key frames");
        detail::checkCovisTable(fn, (size_t)nkf, kfPoint, npoints, pointBad, obs, graph.kfOrder);
        if (kpPoint.size() > 16000) fail("more than 16000 slots");
        for (int32_t p : kpPoint) if (p < -1 || p >= (int64_t)npoints) fail("a slot names a point out of range");
        if (lkfCap < 1 || lkfCap > PGORB_COVIS_MAX_KF || qcap < 1 || qcap > 16000 || nbest < 0 || maxLocal < 0)
            fail("lkfCap outside 1..PGORB_COVIS_MAX_KF, qcap outside 1..16000, or a negative nbest / maxLocal");
        if (!kfBad.empty() && kfBad.size() != (size_t)nkf) fail("kfBad needs one flag per key frame");
        if (prevLocalKf) {
            if ((int64_t)prevLocalKf->size() > lkfCap) fail("the previous list is longer than lkfCap");
            for (int32_t f : *prevLocalKf) if (f < 0 || f >= nkf) fail("a previous key frame is out of range");
        }
        for (int f = 0; f < nkf; f++) {
            if (graph.nord[f] < 0 || graph.nord[f] > cc || graph.parent[f] < -1 || graph.parent[f] >= nkf) fail("an ordered row or a parent is out of range");
            for (int t = 0; t < graph.nord[f]; t++)
                if (graph.ordKf[(size_t)f * cc + t] < 0 || graph.ordKf[(size_t)f * cc + t] >= nkf) fail("an ordered entry is out of range");
        }
        std::vector<const int32_t*> slots((size_t)nkf + 1, nullptr);
        std::vector<int32_t> n((size_t)nkf + 1, 0);
        for (int f = 0; f < nkf; f++) { slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size(); }
        LocalMapResult r;
        r.kpPoint.assign(kpPoint.size() + 1, -1);
        r.localKf.assign((size_t)lkfCap, 0);
        r.queries.assign((size_t)qcap, 0);
        int32_t nlocal = 0, nq = 0, ref = -1, status = 0;
        const int rc = pgorb_update_local_map(ctx_, nkf, slots.data(), n.data(), kfBad.empty() ? nullptr : kfBad.data(), kpPoint.data(), (int)kpPoint.size(),
                                              (int)npoints, pointBad.empty() ? nullptr : pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(), cc,
                                              graph.ordKf.data(), graph.nord.data(), graph.parent.data(), graph.kfOrder.empty() ? nullptr : graph.kfOrder.data(),
                                              nbest, maxLocal, prevLocalKf ? (int)prevLocalKf->size() : -1,
                                              prevLocalKf && !prevLocalKf->empty() ? prevLocalKf->data() : nullptr, r.kpPoint.data(), lkfCap,
                                              r.localKf.data(), &nlocal, &ref, qcap, r.queries.data(), &nq, &status);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        r.kpPoint.resize(kpPoint.size()); r.localKf.resize((size_t)nlocal); r.queries.resize((size_t)nq);
        r.refKf = ref; r.status = status;
        return r;
    }
    // The pose the first search of a frame starts from: UpdateLastFrame (Tracking.cc:792-798) from lastRecord = mlTrajectory.back()
    // and the key-frame poses, then mVelocity * mLastFrame.mTcw (:866) in PGORB_TRACK_MOTION_MODEL; mLastFrame.mTcw (:764) in
    // PGORB_TRACK_REFERENCE_KF.  `state` is updated; returns the PGORB_TRACK_* status (with one, poseOut is the state's last pose).
    int PredictPose(pgorb_track_state& state, int mode, const std::vector<pgorb_kf_pose>& kfPoses, const pgorb_trajectory_record* lastRecord,
                    pgorb_kf_pose& poseOut)
    {
        const char* fn = "Tracking::PredictPose";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        if (mode != PGORB_TRACK_MOTION_MODEL && mode != PGORB_TRACK_REFERENCE_KF) fail("an unknown mode");
        if (kfPoses.size() > PGORB_COVIS_MAX_KF) fail("more than PGORB_COVIS_MAX_KF key frames");
        const int rc = pgorb_track_predict(ctx_, mode, &state, lastRecord, (int)kfPoses.size(), kfPoses.data(), &poseOut);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        return rc;
    }
    // The end of Tracking::Track (:432-440, :493, :497-506): the motion model, the record appended at trajectory[count] (the vector's
    // size is the capacity) and mLastFrame.  Returns the PGORB_TRACK_* status (PGORB_TRACK_FULL | PGORB_TRACK_BAD_INDEX: nothing changed).
    int CommitFrame(pgorb_track_state& state, const pgorb_kf_pose& pose, bool ok, int refKf, double frameTime, int64_t frameId,
                    const std::vector<pgorb_kf_pose>& kfPoses, std::vector<pgorb_trajectory_record>& trajectory, int32_t& count)
    {
        const char* fn = "Tracking::CommitFrame";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        if (kfPoses.size() > PGORB_COVIS_MAX_KF || trajectory.size() > (size_t)PGORB_TRAJ_MAX_RECORDS)
            fail("more than PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
        if (count < 0) fail("a negative count");
        const int rc = pgorb_track_commit(ctx_, &state, &pose, ok ? 1 : 0, refKf, frameTime, frameId, (int)kfPoses.size(), kfPoses.data(), trajectory.data(),
                                          (int)trajectory.size(), &count);
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        return rc;
    }
 private:
    pgorb_ctx* ctx_;
};

namespace detail {
// what both cullings reject of the masked observation lists beyond checkCovisTable
inline void checkCullTable(const char* fn, const std::vector<std::vector<int32_t>>& kfPoint, size_t npoints, const std::vector<uint8_t>& pointBad,
                           const MapPointObservations& O, const std::vector<uint8_t>& obsLive, const std::vector<int32_t>& kfOrder)
{
    auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
    if (pointBad.size() != npoints) fail("pointBad needs one flag per point");
    checkCovisTable(fn, kfPoint.size(), kfPoint, npoints, pointBad, O, kfOrder);
    const size_t m = (size_t)O.obsStart[npoints];
    if (O.obsIdx.size() < m || obsLive.size() < m) fail("obsIdx and obsLive need one entry per observation");
    for (size_t k = 0; k < m; k++)
        if (O.obsIdx[k] < 0 || O.obsIdx[k] >= (int64_t)kfPoint[O.obsFrame[k]].size()) fail("an observation names a keypoint out of range");
}
}  // namespace detail

inline int LocalMapping::MapPointCulling(std::vector<std::vector<int32_t>>& kfPoint, std::vector<uint8_t>& pointBad, const MapPointObservations& obs,
                                         std::vector<uint8_t>& obsLive, const std::vector<int32_t>& firstKfId, const std::vector<int32_t>& visible,
                                         const std::vector<int32_t>& found, const std::vector<int32_t>& recent, int curKfId, int thObs,
                                         std::vector<int32_t>& action, std::vector<int32_t>& survivors, std::array<int32_t, PGORB_CULL_INFO>* info)
{
    const char* fn = "LocalMapping::MapPointCulling";
    auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
    const size_t np = pointBad.size(), nkf = kfPoint.size();
    detail::checkCullTable(fn, kfPoint, np, pointBad, obs, obsLive, {});
    if (firstKfId.size() != np || visible.size() != np || found.size() != np) fail("firstKfId, visible and found need one entry per point");
    std::vector<uint8_t> listed(np + 1, 0);
    for (int32_t p : recent) {
        if (p < 0 || p >= (int64_t)np) fail("a recent entry is out of range");
        if (listed[p]) fail("the recent list names a point twice");
        listed[p] = 1;
    }
    std::vector<int32_t*> slots(nkf + 1, nullptr);
    std::vector<int32_t> n(nkf + 1, 0);
    for (size_t f = 0; f < nkf; f++) { slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size(); }
    const size_t nr = recent.size();
    action.assign(nr + 1, 0);
    survivors.assign(nr + 1, 0);
    int32_t nout = 0;
    std::array<int32_t, PGORB_CULL_INFO> inf{};
    const int rc = pgorb_map_point_culling(ctx_, (int)nkf, slots.data(), n.data(), (int)np, pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(),
                                           obs.obsIdx.data(), obsLive.data(), firstKfId.data(), visible.data(), found.data(), (int)nr,
                                           nr ? recent.data() : n.data(), curKfId, thObs, action.data(), survivors.data(), &nout, inf.data());
    if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
    action.resize(nr);
    survivors.resize((size_t)nout);
    if (info) *info = inf;
    return rc;
}

inline int LocalMapping::KeyFrameCulling(CovisibilityGraph& graph, int curKf, const std::vector<std::vector<int32_t>>& octaves,
                                         std::vector<std::vector<int32_t>>& kfPoint, std::vector<uint8_t>& pointBad, const MapPointObservations& obs,
                                         std::vector<uint8_t>& obsLive, std::vector<int32_t>& refObs, const std::vector<uint8_t>& kfNotErase,
                                         std::vector<uint8_t>& kfBad, std::vector<uint8_t>& kfToBeErased, int listCap, std::vector<int32_t>& record,
                                         std::vector<int32_t>& rowStatus, std::array<int32_t, PGORB_CULL_INFO>* info)
{
    const char* fn = "LocalMapping::KeyFrameCulling";
    auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
    const int nkf = graph.nkf(), cc = graph.connCap();
    const size_t np = pointBad.size();
    if (kfPoint.size() != (size_t)nkf) fail("one slot array per key frame");
    detail::checkCullTable(fn, kfPoint, np, pointBad, obs, obsLive, graph.kfOrder);
    if (curKf < 0 || curKf >= nkf) fail("curKf is out of range");
    if (listCap < 1) fail("listCap < 1");
    if (octaves.size() != (size_t)nkf) fail("one octave array per key frame");
    for (int f = 0; f < nkf; f++) if (octaves[f].size() != kfPoint[f].size()) fail("one octave per slot");
    if (refObs.size() != np) fail("refObs needs one entry per point");
    for (size_t p = 0; p < np; p++) {
        const int len = obs.obsStart[p + 1] - obs.obsStart[p];
        if (len && (refObs[p] < -1 || refObs[p] >= len)) fail("refObs lies outside the point's list");
    }
    if (kfBad.size() != (size_t)nkf || kfToBeErased.size() != (size_t)nkf || (!kfNotErase.empty() && kfNotErase.size() != (size_t)nkf) ||
        (!graph.kfId0.empty() && graph.kfId0.size() != (size_t)nkf))
        fail("kfBad, kfToBeErased, kfNotErase and kfId0 need one flag per key frame");
    graph.checkRows(fn);
    std::vector<std::vector<pgorb_keypoint>> keys((size_t)nkf);
    std::vector<const pgorb_keypoint*> kps((size_t)nkf + 1, nullptr);
    std::vector<int32_t*> slots((size_t)nkf + 1, nullptr);
    std::vector<int32_t> n((size_t)nkf + 1, 0);
    for (int f = 0; f < nkf; f++) {
        keys[f].assign(octaves[f].size() + 1, pgorb_keypoint{});
        for (size_t i = 0; i < octaves[f].size(); i++) keys[f][i].octave = octaves[f][i];
        kps[f] = keys[f].data(); slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size();
    }
    record.assign((size_t)listCap * 4, 0);
    rowStatus.assign((size_t)std::max(nkf, 1), 0);
    std::array<int32_t, PGORB_CULL_INFO> inf{};
    const int rc = pgorb_keyframe_culling(ctx_, nkf, kps.data(), slots.data(), n.data(), (int)np, pointBad.data(), obs.obsStart.data(), obs.obsFrame.data(),
                                          obs.obsIdx.data(), obsLive.data(), refObs.data(), graph.kfOrder.empty() ? nullptr : graph.kfOrder.data(),
                                          graph.kfId0.empty() ? nullptr : graph.kfId0.data(), kfNotErase.empty() ? nullptr : kfNotErase.data(),
                                          kfBad.data(), kfToBeErased.data(), curKf, cc, graph.connKf.data(), graph.connW.data(), graph.nconn.data(),
                                          graph.ordKf.data(), graph.ordW.data(), graph.nord.data(), graph.parent.data(), listCap, record.data(),
                                          rowStatus.data(), inf.data());
    if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
    record.resize((inf[0] & PGORB_CULL_LIMIT) ? 0 : (size_t)inf[1] * 4);
    rowStatus.resize((size_t)nkf);
    if (info) *info = inf;
    return rc;
}

struct LoopCorrection {
    std::vector<uint8_t> hasCorrected, hasNonCorrected;       // CorrectedSim3 / NonCorrectedSim3 as pgorb_optimize_essential_graph takes them
    std::vector<pgorb_sim3d> corrected, nonCorrected;
    std::vector<pgorb_kf_pose> poses;
    std::vector<int32_t> correctedBy, pointRefKf;             // mnCorrectedReference (-1 = not corrected); the essential graph's point_ref_kf
    std::array<int32_t, PGORB_LC_INFO> info{};
};
struct MapUpdate {
    std::vector<pgorb_kf_pose> poses;
    std::vector<uint8_t> kfUpdated, pointUpdated;
    std::array<int32_t, PGORB_MU_INFO> info{};
};

// The two map rewrites of loop closing (LoopClosing.cc:438-516 and :679-742); include/pgorb.h states both contracts.  Every input
// the single calls refuse is a std::invalid_argument here, before the library is called.
class LoopClosing {
 public:
    explicit LoopClosing(pgorb_ctx* ctx) : ctx_(ctx) {}
    // CorrectLoop's propagation.  octaves[f] = mvKeysUn[i].octave, poses, curKf, scw = mg2oScw, connected = mvpCurrentConnectedKFs
    // (an entry that is negative, out of range or curKf is skipped), kfPoint[f] the slots, the table (points corrected IN PLACE),
    // obs with refObs, refKf[p] = GetReferenceKeyFrame() or -1, kfOrder the address ranks (empty = index order).  Returns the
    // number of points corrected.
    int CorrectLoopPoses(const std::vector<std::vector<int32_t>>& octaves, const std::vector<pgorb_kf_pose>& poses, int curKf, const pgorb_sim3d& scw,
                         const std::vector<int32_t>& connected, const std::vector<std::vector<int32_t>>& kfPoint, std::vector<pgorb_map_point>& points,
                         const std::vector<uint8_t>& pointBad, const MapPointObservations& obs, const std::vector<int32_t>& refKf,
                         const std::vector<int32_t>& kfOrder, LoopCorrection& out)
    {
        const char* fn = "LoopClosing::CorrectLoopPoses";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        const size_t nkf = kfPoint.size(), np = points.size();
        detail::checkCovisTable(fn, nkf, kfPoint, np, pointBad, obs, kfOrder);
        if (curKf < 0 || curKf >= (int64_t)nkf) fail("curKf is out of range");
        if (poses.size() != nkf || octaves.size() != nkf) fail("poses and octaves need one entry per key frame");
        for (size_t f = 0; f < nkf; f++) {
            if (octaves[f].size() != kfPoint[f].size()) fail("one octave per slot");
            if (!poseFinite(poses[f])) fail("a pose is not finite");
        }
        for (int k = 0; k < 4; k++) if (!std::isfinite(scw.r[k])) fail("scw is not finite");
        for (int k = 0; k < 3; k++) if (!std::isfinite(scw.t[k])) fail("scw is not finite");
        if (!std::isfinite(scw.s)) fail("scw is not finite");
        if (!(scw.s > 0.0)) fail("the scale of scw is not positive");
        if (connected.size() > PGORB_COVIS_MAX_KF) fail("more than PGORB_COVIS_MAX_KF list entries");
        const size_t m = (size_t)obs.obsStart[np];
        if (obs.obsIdx.size() < m) fail("obsIdx is shorter than obsStart says");
        for (size_t k = 0; k < m; k++)
            if (obs.obsIdx[k] < 0 || obs.obsIdx[k] >= (int64_t)kfPoint[obs.obsFrame[k]].size()) fail("an observation names a keypoint out of range");
        if (obs.refObs.size() != np || refKf.size() != np) fail("refObs and refKf need one entry per point");
        for (size_t p = 0; p < np; p++) {
            const int len = obs.obsStart[p + 1] - obs.obsStart[p];
            if (!posFinite(points[p].pos)) fail("a point is not finite");
            if (refKf[p] < -1 || refKf[p] >= (int64_t)nkf) fail("refKf is out of range");
            if (!(!pointBad.empty() && pointBad[p]) && len > 0 && len <= PGORB_MP_MAX_OBS && (obs.refObs[p] < 0 || obs.refObs[p] >= len))
                fail("refObs lies outside the point's list");
        }
        std::vector<std::vector<pgorb_keypoint>> keys(nkf);
        std::vector<const pgorb_keypoint*> kps(nkf + 1, nullptr);
        std::vector<const int32_t*> slots(nkf + 1, nullptr);
        std::vector<int32_t> n(nkf + 1, 0);
        for (size_t f = 0; f < nkf; f++) {
            keys[f].assign(octaves[f].size() + 1, pgorb_keypoint{});
            for (size_t i = 0; i < octaves[f].size(); i++) keys[f][i].octave = octaves[f][i];
            kps[f] = keys[f].data(); slots[f] = kfPoint[f].data(); n[f] = (int32_t)kfPoint[f].size();
        }
        out.hasCorrected.assign(nkf, 0); out.hasNonCorrected.assign(nkf, 0);
        out.corrected.assign(nkf, pgorb_sim3d{}); out.nonCorrected.assign(nkf, pgorb_sim3d{});
        out.poses.assign(nkf, pgorb_kf_pose{});
        out.correctedBy.assign(np + 1, -1); out.pointRefKf.assign(np + 1, -1);
        std::vector<pgorb_map_point> one(1);
        const int rc = pgorb_correct_loop_poses(ctx_, (int)nkf, kps.data(), n.data(), poses.data(), curKf, &scw, (int)connected.size(),
                                                connected.empty() ? n.data() : connected.data(), kfOrder.empty() ? nullptr : kfOrder.data(), slots.data(),
                                                (int)np, np ? points.data() : one.data(), pointBad.empty() ? nullptr : pointBad.data(), obs.obsStart.data(),
                                                obs.obsFrame.data(), obs.obsIdx.data(), np ? obs.refObs.data() : n.data(), np ? refKf.data() : n.data(),
                                                out.hasCorrected.data(), out.corrected.data(), out.hasNonCorrected.data(), out.nonCorrected.data(),
                                                out.poses.data(), out.correctedBy.data(), out.pointRefKf.data(), out.info.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        out.correctedBy.resize(np); out.pointRefKf.resize(np);
        return rc;
    }
    // The map update after global bundle adjustment.  poses = the poses as they stand (mTcwBefGBA), posesGba / kfDone / posGba
    // [np][3] / pointDone as GlobalBundleAdjustment leaves them, parent[f] or -1, kfOrigin[f] = is in mvpKeyFrameOrigins, kfBad and
    // pointBad may be empty, refKf[p] or -1; points[].pos is updated IN PLACE.  Returns the number of key frames updated.
    int UpdateMapAfterGBA(const std::vector<pgorb_kf_pose>& poses, const std::vector<pgorb_kf_pose>& posesGba, const std::vector<uint8_t>& kfDone,
                          const std::vector<int32_t>& parent, const std::vector<uint8_t>& kfOrigin, const std::vector<uint8_t>& kfBad,
                          std::vector<pgorb_map_point>& points, const std::vector<float>& posGba, const std::vector<uint8_t>& pointDone,
                          const std::vector<uint8_t>& pointBad, const std::vector<int32_t>& refKf, MapUpdate& out)
    {
        const char* fn = "LoopClosing::UpdateMapAfterGBA";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        const size_t nkf = parent.size(), np = points.size();
        if (nkf > PGORB_COVIS_MAX_KF) fail("more than PGORB_COVIS_MAX_KF key frames");
        if (poses.size() != nkf || posesGba.size() != nkf || kfDone.size() != nkf || kfOrigin.size() != nkf || (!kfBad.empty() && kfBad.size() != nkf))
            fail("poses, posesGba, kfDone, kfOrigin and kfBad need one entry per key frame");
        if (posGba.size() != 3 * np || pointDone.size() != np || refKf.size() != np || (!pointBad.empty() && pointBad.size() != np))
            fail("posGba, pointDone, refKf and pointBad need one entry per point");
        for (size_t k = 0; k < nkf; k++) {
            if (parent[k] < -1 || parent[k] >= (int64_t)nkf) fail("a parent is out of range");
            if (!poseFinite(poses[k]) || (kfDone[k] && !poseFinite(posesGba[k]))) fail("a pose is not finite");
        }
        std::vector<int32_t> mark(nkf + 1, -1);
        for (size_t k = 0; k < nkf; k++) {
            int cur = (int)k;
            while (cur >= 0 && mark[cur] < 0) { mark[cur] = (int32_t)k; cur = parent[cur]; }
            if (cur >= 0 && mark[cur] == (int32_t)k) fail("the parents form a cycle");
        }
        for (size_t p = 0; p < np; p++) {
            if (refKf[p] < -1 || refKf[p] >= (int64_t)nkf) fail("refKf is out of range");
            if (!posFinite(points[p].pos) || (pointDone[p] && !posFinite(&posGba[3 * p]))) fail("a point is not finite");
        }
        out.poses.assign(nkf + 1, pgorb_kf_pose{}); out.kfUpdated.assign(nkf + 1, 0); out.pointUpdated.assign(np + 1, 0);
        const int rc = pgorb_global_ba_map_update(ctx_, (int)nkf, poses.data(), posesGba.data(), kfDone.data(), parent.data(), kfOrigin.data(),
                                                  kfBad.empty() ? nullptr : kfBad.data(), (int)np, points.data(), posGba.data(), pointDone.data(),
                                                  pointBad.empty() ? nullptr : pointBad.data(), refKf.data(), out.poses.data(), out.kfUpdated.data(),
                                                  out.pointUpdated.data(), out.info.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        out.poses.resize(nkf); out.kfUpdated.resize(nkf); out.pointUpdated.resize(np);
        return rc;
    }
 private:
    static bool poseFinite(const pgorb_kf_pose& P)
    {
        for (float v : P.Tcw) if (!std::isfinite(v)) return false;
        return std::isfinite(P.Ow[0]) && std::isfinite(P.Ow[1]) && std::isfinite(P.Ow[2]);
    }
    static bool posFinite(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
    pgorb_ctx* ctx_;
};

// what System::GetTrajectory returns, in the layout pgorb_smooth_heading_directions / pgorb_trajectory_pca take
struct TrajectoryResult {
    std::vector<double> quatWxyz, translation;       // [n][4], [n][3]
    std::vector<int64_t> timeUsec, frameId;
    std::vector<uint8_t> isLost;
    std::vector<int32_t> status;                     // PGORB_TRAJ_BROKEN per record
    std::array<int32_t, PGORB_TRAJ_INFO> info{};     // status, origin key frame, broken records, records
};

class System {
 public:
    explicit System(pgorb_ctx* ctx) : ctx_(ctx) {}
    // System::GetTrajectory (System.cc:371-412) over the key-frame table (poses, kfBad, parent, kfId = mnId, tcp [nkf][12] = mTcp rows
    // 0-2, read where kfBad is set) and one tracker's records.
    TrajectoryResult GetTrajectory(const std::vector<pgorb_kf_pose>& poses, const std::vector<uint8_t>& kfBad, const std::vector<int32_t>& parent,
                                   const std::vector<uint64_t>& kfId, const std::vector<float>& tcp, const std::vector<pgorb_trajectory_record>& trajectory)
    {
        const char* fn = "System::GetTrajectory";
        auto fail = [&](const char* what) { throw std::invalid_argument(std::string(fn) + ": " + what); };
        const size_t nkf = parent.size(), n = trajectory.size();
        if (nkf > PGORB_COVIS_MAX_KF || n > (size_t)PGORB_TRAJ_MAX_RECORDS) fail("more than PGORB_COVIS_MAX_KF key frames or PGORB_TRAJ_MAX_RECORDS records");
        if (poses.size() != nkf || kfBad.size() != nkf || kfId.size() != nkf || tcp.size() != 12 * nkf) fail("poses, kfBad, kfId and tcp need one entry per key frame");
        bool live = false;
        for (size_t k = 0; k < nkf; k++) {
            if (!kfBad[k]) live = true;
            else if (parent[k] < 0 || parent[k] >= (int64_t)nkf) fail("a bad key frame has no parent or one out of range");
        }
        if (!live) fail("no live key frame");
        for (const pgorb_trajectory_record& r : trajectory) {
            const double us = r.frame_time * 1e6;
            if (!std::isfinite(r.frame_time) || !(us >= -9223372036854775808.0 && us < 9223372036854775808.0))
                fail("a frame time is not finite or outside int64 microseconds");
            if (!r.lost && (r.ref_kf < 0 || r.ref_kf >= (int64_t)nkf)) fail("a record's reference key frame is out of range");
        }
        TrajectoryResult out;
        out.quatWxyz.assign(4 * n + 4, 0.0); out.translation.assign(3 * n + 3, 0.0); out.timeUsec.assign(n + 1, 0); out.frameId.assign(n + 1, 0);
        out.isLost.assign(n + 1, 0); out.status.assign(n + 1, 0);
        const int rc = pgorb_get_trajectory(ctx_, (int)nkf, poses.data(), kfBad.data(), parent.data(), kfId.data(), tcp.data(), (int)n, trajectory.data(),
                                            out.quatWxyz.data(), out.translation.data(), out.timeUsec.data(), out.frameId.data(), out.isLost.data(),
                                            out.status.data(), out.info.data());
        if (rc < 0) throw std::runtime_error(pgorb_last_error(ctx_));
        out.quatWxyz.resize(4 * n); out.translation.resize(3 * n); out.timeUsec.resize(n); out.frameId.resize(n); out.isLost.resize(n); out.status.resize(n);
        return out;
    }
 private:
    pgorb_ctx* ctx_;
};

}  // namespace pgorb
