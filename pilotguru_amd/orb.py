"""Host-side mirror of the reference's ORB interface over the C ABI.

Names, argument meaning and error behaviour follow
  ORB_SLAM2::ORBextractor   thirdparty/orb-slam2/include/ORBextractor.h:44-110
  ORB_SLAM2::ORBmatcher     thirdparty/orb-slam2/include/ORBmatcher.h:44 (DescriptorDistance)
so the parity tests read like tests of the reference classes.  All compute happens in
libpgorb.so (HIP, gfx950); numpy / torch only carry buffers.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _arr(x, dtype, n, name, width=None):
    """x as a C-contiguous `dtype` array of exactly n entries, or n rows of `width` (descriptors: 32 bytes, vbPrevMatched: 2
    floats); anything else is a ValueError.  The library reads exactly that much through the pointer."""
    a = np.ascontiguousarray(x, dtype)
    if a.shape != ((n,) if width is None else (n, width)):
        raise ValueError("%s: shape %s, expected %s" % (name, a.shape, (n,) if width is None else (n, width)))
    return a


def _frame(F, name):
    """A frame's keypoints and descriptors, checked against F.N."""
    return (_arr(F.mvKeysUndistorted, KEYPOINT_DTYPE, F.N, name + " keypoints"),
            _arr(F.mDescriptors, np.uint8, F.N, name + " descriptors", 32))


def _mask(m, n, name):
    """A per-keypoint flag array of n entries; None = all zero."""
    return np.zeros(max(n, 1), np.uint8) if m is None else _arr(m, np.uint8, n, name)


def _featvec(fv, name):
    """(nodes, starts, features) of a FeatureVector: nfv + 1 starts and at least starts[-1] features (the library reads
    that many)."""
    fv = [np.ascontiguousarray(fv[0], np.uint32).reshape(-1), np.ascontiguousarray(fv[1], np.int32).reshape(-1),
          np.ascontiguousarray(fv[2], np.uint32).reshape(-1)]
    if len(fv[1]) != len(fv[0]) + 1 or len(fv[2]) < int(fv[1][-1]):
        raise ValueError("%s: FeatureVector arrays of inconsistent lengths" % name)
    return fv


class ORBextractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) (ORBextractor.h:51-52).

    Extra keyword arguments size the device context (largest frame, frames per batch, GPU).
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, *,
                 max_width=1920, max_height=1080, max_batch=1, device=0, blur_tie_mode=0):
        self._L = _lib.lib()
        self.nfeatures, self.nlevels = int(nfeatures), int(nlevels)
        self.scaleFactor = float(scaleFactor)
        self.max_batch = int(max_batch)
        self.device = int(device)
        prm = _lib.PgorbParams(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                               max_width, max_height, max_batch, device, blur_tie_mode)
        h = C.c_void_p()
        rc = self._L.pgorb_create(C.byref(prm), C.byref(h))
        if rc != 0:
            raise _lib.PgorbError(rc, self._L.pgorb_last_error(None).decode())
        self._h = h
        self._streams = weakref.WeakSet()             # FrameStreams of this context: pgorb_destroy takes them along

    def close(self):
        if getattr(self, "_h", None):
            for st in list(self._streams):            # the C context destroys its live streams: their handles die with it
                st._s = None
            self._L.pgorb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise _lib.PgorbError(rc, self._L.pgorb_last_error(self._h).decode())
        return rc

    # ---- getters, ORBextractor.h:63-83 -------------------------------------------------
    def GetLevels(self):
        return self._L.pgorb_levels(self._h)

    def GetScaleFactor(self):
        return self.scaleFactor

    def _tables(self):
        n = self.nlevels + 1
        t = [np.zeros(n, np.float32) for _ in range(4)]
        fp = C.POINTER(C.c_float)
        self._check(self._L.pgorb_scale_tables(self._h, *[a.ctypes.data_as(fp) for a in t]))
        return t

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        out = np.zeros(self.nlevels + 1, np.int32)
        self._check(self._L.pgorb_features_per_level(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def max_keypoints(self, w, h):
        return self._check(self._L.pgorb_max_keypoints(self._h, w, h))

    # ---- operator(), ORBextractor.h:59-61 -----------------------------------------------
    def __call__(self, image, mask=None):
        """(keypoints, descriptors) of one CV_8UC1 image.  `mask` is ignored, as in the
        reference (ORBextractor.h:58).  An empty image returns empty outputs (:1045)."""
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise TypeError("image must be CV_8UC1 (2-D uint8)")      # assert(type==CV_8UC1) :1049
        out = self.extract_batch([image])
        return out[0]

    def extract_batch(self, frames):
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        h, w = frames[0].shape
        cap = self.max_keypoints(w, h)
        nfr = len(frames)
        kps = np.zeros((nfr, cap), KEYPOINT_DTYPE)
        desc = np.zeros((nfr, cap, 32), np.uint8)
        n = np.zeros(nfr, np.int32)
        ptrs = (C.c_void_p * nfr)(*[f.ctypes.data for f in frames])
        self._check(self._L.pgorb_extract_batch(self._h, ptrs, nfr, w, h, w, _p(kps), _p(desc), cap,
                                                n.ctypes.data_as(C.POINTER(C.c_int32))))
        return [(kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(nfr)]

    def extract_batch_device(self, frames_u8, kps_out=None, desc_out=None, n_out=None, stream=None):
        """Resident path: `frames_u8` is a CUDA(HIP) torch uint8 tensor [B, H, W].  Returns torch
        tensors (kps [B,cap,7] float32 view of pgorb_keypoint, desc [B,cap,32] u8, n [B] i32);
        asynchronous on `stream` (default: torch's current stream)."""
        import torch
        B, H, W = frames_u8.shape
        cap = self.max_keypoints(W, H)
        dev = frames_u8.device
        if kps_out is None:
            kps_out = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
            desc_out = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
            n_out = torch.empty((B,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.pgorb_extract_batch_device(
            self._h, C.c_void_p(frames_u8.data_ptr()), B, W, H, frames_u8.stride(1),
            frames_u8.stride(0), C.c_void_p(kps_out.data_ptr()), C.c_void_p(desc_out.data_ptr()),
            cap, C.c_void_p(n_out.data_ptr()), C.c_void_p(s)))
        return kps_out, desc_out, n_out

    def extract_batch_color_device(self, frames_rgb, rgb_order=True, stream=None):
        """`frames_rgb`: CUDA(HIP) torch uint8 tensor [B, H, W, C], C = 3 or 4; fuses
        Tracking::GrabImageMonocular's cvtColor (Tracking.cc:247-260) in front of the extractor."""
        import torch
        B, H, W, Cn = frames_rgb.shape
        cap = self.max_keypoints(W, H)
        dev = frames_rgb.device
        kps = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
        desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
        n = torch.empty((B,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.pgorb_extract_batch_color_device(
            self._h, C.c_void_p(frames_rgb.data_ptr()), B, W, H, frames_rgb.stride(1), frames_rgb.stride(0), Cn,
            int(bool(rgb_order)), C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap,
            C.c_void_p(n.data_ptr()), C.c_void_p(s)))
        return kps, desc, n

    def extract_batch_ingest_device(self, frames, rgb_order=True, rotate_degrees=0, vertical_flip=False,
                                    horizontal_flip=False, stream=None):
        """`frames`: CUDA(HIP) torch uint8 tensor [B, H, W] (grey) or [B, H, W, C] (C = 3 or 4) exactly
        as decoded; applies the reader's rotation (0/90/180/270, image_sequence_reader.cc:186-205)
        and flips (:53-58) and Tracking's grey conversion on the device, then extracts."""
        import torch
        if frames.dim() == 3:
            B, H, W = frames.shape
            Cn = 1
        else:
            B, H, W, Cn = frames.shape
        ow, oh = (H, W) if rotate_degrees in (90, 270) else (W, H)
        cap = self.max_keypoints(ow, oh)
        dev = frames.device
        kps = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
        desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
        n = torch.empty((B,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.pgorb_extract_batch_ingest_device(
            self._h, C.c_void_p(frames.data_ptr()), B, W, H, frames.stride(1), frames.stride(0), Cn,
            int(bool(rgb_order)), int(rotate_degrees), int(bool(vertical_flip)), int(bool(horizontal_flip)),
            C.c_void_p(kps.data_ptr()), C.c_void_p(desc.data_ptr()), cap, C.c_void_p(n.data_ptr()), C.c_void_p(s)))
        return kps, desc, n

    def check_async(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        self._check(self._L.pgorb_check_async(self._h, C.c_void_p(s)))

    def match_batch_device(self, desc, n, pair_query, pair_train, out=None, stream=None):
        """best/second-best Hamming match of frame pair_query[p] against pair_train[p]."""
        import torch
        B, cap, _ = desc.shape
        npairs = pair_query.numel()
        dev = desc.device
        if out is None:
            out = (torch.empty((npairs, cap), dtype=torch.int32, device=dev),
                   torch.empty((npairs, cap), dtype=torch.int16, device=dev),
                   torch.empty((npairs, cap), dtype=torch.int16, device=dev))
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.pgorb_match_batch_device(
            self._h, C.c_void_p(desc.data_ptr()), C.c_void_p(n.data_ptr()), cap,
            C.c_void_p(pair_query.data_ptr()), C.c_void_p(pair_train.data_ptr()), npairs,
            C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
            C.c_void_p(out[2].data_ptr()), C.c_void_p(s)))
        return out

    def log_scale_factor(self):
        """Frame::mfLogScaleFactor = log(mfScaleFactor) (Frame.cc:188) under the library's log contract."""
        return float(self._L.pgorb_log_scale_factor(self._h))

    def predict_scale(self, max_distance, current_dist):
        """MapPoint::PredictScale(currentDist, pF) (src/MapPoint.cc:516-531)."""
        return self._check(self._L.pgorb_predict_scale(self._h, float(max_distance), float(current_dist)))

    def set_option(self, key, value):
        """Measurement switches of the library (include/pgorb.h: pgorb_set_option)."""
        self._check(self._L.pgorb_set_option(self._h, key.encode(), int(value)))

    def matcher_name(self, cap_per_frame):
        return "popcount" if self._L.pgorb_matcher_is_popcount(self._h, int(cap_per_frame)) else "mfma_fp4"

    def get_option(self, key):
        v = self._L.pgorb_get_option(self._h, key.encode())
        if v == -2147483648:                                     # PGORB_OPTION_UNKNOWN
            raise KeyError(key)
        return v

    def fast_kernel_name(self):
        """Name of the K2 kernel (for bench.py's roofline object)."""
        return "k_fast_cells"

    STAGES = ("pyramid", "fast", "quadtree", "describe", "match")

    def profile_begin(self, max_calls):
        self._check(self._L.pgorb_profile_begin(self._h, max_calls))

    def profile_read(self):
        """{stage: mean ms per call} measured with HIP events on the launch stream."""
        ms = (C.c_double * 5)()
        n = self._check(self._L.pgorb_profile_read(self._h, ms))
        return n, dict(zip(self.STAGES, list(ms)))

    # ---- stage taps (parity tests) --------------------------------------------------------
    def debug_level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        self._check(self._L.pgorb_debug_level_size(self._h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def debug_level_image(self, frame, level):
        w, h = self.debug_level_size(level)
        out = np.zeros((h, w), np.uint8)
        self._check(self._L.pgorb_debug_level_image(self._h, frame, level, _p(out)))
        return out

    def debug_level_candidates(self, frame, level):
        w, h = self.debug_level_size(level)
        cap = w * h // 2 + 64
        x, y, r = (np.zeros(cap, np.int32) for _ in range(3))
        n = self._check(self._L.pgorb_debug_level_candidates(self._h, frame, level, _p(x), _p(y), _p(r), cap))
        return x[:n].copy(), y[:n].copy(), r[:n].copy()

    def debug_level_keypoints(self, frame, level):
        return self._check(self._L.pgorb_debug_level_keypoints(self._h, frame, level))

    ARENAS = ("stageA", "pinned", "stageSfi", "stageOut", "xdesc", "outBlk", "vocab", "plan_pyr", "plan_tables")

    def debug_arena(self, name):
        """(address, bytes) of one of the context's shared arenas (pgorb_debug_arena; read-only, for the session tests)."""
        ptr, n = C.c_void_p(), C.c_int64()
        self._check(self._L.pgorb_debug_arena(self._h, self.ARENAS.index(name), C.byref(ptr), C.byref(n)))
        return ptr.value or 0, n.value

    def debug_host_graph(self):
        """(how the last host-frame extract ran: 0 direct, 1 captured, 2 replayed; the plan epoch)."""
        last, epoch = C.c_int32(), C.c_int32()
        self._check(self._L.pgorb_debug_host_graph(self._h, C.byref(last), C.byref(epoch)))
        return last.value, epoch.value

    # ---- Hamming (device) -------------------------------------------------------------------
    def hamming_matrix(self, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros((len(a), len(b)), np.uint16)
        self._check(self._L.pgorb_hamming_matrix(self._h, _p(a), len(a), _p(b), len(b), _p(out)))
        return out

    def hamming_best2(self, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        bi = np.zeros(len(a), np.int32)
        b1 = np.zeros(len(a), np.uint16)
        b2 = np.zeros(len(a), np.uint16)
        self._check(self._L.pgorb_hamming_best2(self._h, _p(a), len(a), _p(b), len(b), _p(bi), _p(b1), _p(b2)))
        return bi, b1, b2


class Frame:
    """The part of ORB_SLAM2::Frame the front end needs (thirdparty/orb-slam2/include/Frame.h):
    mvKeys (== mvKeysUndistorted for k1 == 0), mDescriptors, the image bounds and the 64x48 grid
    (AssignFeaturesToGrid, src/Frame.cc:234-249), built on the GPU."""

    def __init__(self, extractor, image, camera=None, dist_coef=None):
        """camera = (fx, fy, cx, cy), dist_coef = (k1, k2, p1, p2[, k3]) like mK / mDistCoef; without
        them (or with k1 == 0) the keypoints are used as they are (Frame.cc:410-414)."""
        self.ext = extractor
        self.mvKeys, self.mDescriptors = extractor(image)
        self.N = len(self.mvKeys)
        h, w = image.shape
        L = extractor._L
        if camera is not None and dist_coef is not None and float(dist_coef[0]) != 0.0:
            cam = np.ascontiguousarray(camera, np.float32)
            dc = np.zeros(5, np.float32)
            dc[:len(dist_coef)] = dist_coef
            self.mvKeysUndistorted = np.zeros_like(self.mvKeys)                      # UndistortKeyPoints (Frame.cc:408-438)
            if self.N:
                extractor._check(L.pgorb_undistort_keypoints(extractor._h, _p(self.mvKeys), self.N, _p(cam), _p(dc),
                                                             _p(self.mvKeysUndistorted)))
            b = np.zeros(4, np.float32)
            L.pgorb_image_bounds(w, h, _p(cam), _p(dc), _p(b))                       # ComputeImageBounds (Frame.cc:440-467)
            self.bounds = tuple(float(x) for x in b)
        else:
            self.mvKeysUndistorted = self.mvKeys
            self.bounds = (0.0, float(w), 0.0, float(h))      # mnMinX, mnMaxX, mnMinY, mnMaxY (Frame.cc:461-466)
        self.grid_start = np.zeros(64 * 48 + 1, np.int32)
        self.grid_idx = np.zeros(max(self.N, 1), np.int32)
        if self.N:
            extractor._check(L.pgorb_frame_grid(extractor._h, _p(self.mvKeysUndistorted), self.N, *self.bounds,
                                                _p(self.grid_start), _p(self.grid_idx)))

    def grid_cell(self, col, row):
        """mGrid[col][row] as an index array."""
        c = col * 48 + row
        return self.grid_idx[self.grid_start[c]:self.grid_start[c + 1]]


class MapPoints:
    """What the matchers read from a set of ORB_SLAM2::MapPoint (thirdparty/orb-slam2/include/
    MapPoint.h) as arrays: valid (mbTrackInView && !isBad()), projection, predicted level, viewing
    cosine, representative descriptor, Observations() > 0."""

    def __init__(self, valid, proj_x, proj_y, level, view_cos, descriptors, has_obs):
        self.valid = np.ascontiguousarray(valid, np.uint8)
        self.proj_x = np.ascontiguousarray(proj_x, np.float32)
        self.proj_y = np.ascontiguousarray(proj_y, np.float32)
        self.level = np.ascontiguousarray(level, np.int32)
        self.view_cos = np.ascontiguousarray(view_cos, np.float32)
        self.descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        self.has_obs = np.ascontiguousarray(has_obs, np.uint8)


class ORBmatcher:
    """ORBmatcher(nnratio, checkOri) (thirdparty/orb-slam2/include/ORBmatcher.h:40-44)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30               # src/ORBmatcher.cc:38-40

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio, self.mbCheckOrientation = float(nnratio), bool(checkOri)

    def SearchByProjection(self, F, points, th, kp_has_point=None):
        """SearchByProjection(Frame &F, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:46-131).
        Returns (nmatches, assigned) with assigned[i] = index into `points` written to
        F.mvpMapPoints[i], or -1."""
        ext = F.ext
        kp, desc = _frame(F, "F")
        has = _mask(kp_has_point, F.N, "kp_has_point")
        n = len(points.valid)
        q = [_arr(points.valid, np.uint8, n, "valid"), _arr(points.proj_x, np.float32, n, "proj_x"),
             _arr(points.proj_y, np.float32, n, "proj_y"), _arr(points.level, np.int32, n, "level"),
             _arr(points.view_cos, np.float32, n, "view_cos"), _arr(points.descriptors, np.uint8, n, "descriptors", 32),
             _arr(points.has_obs, np.uint8, n, "has_obs")]
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_projection_points(
            ext._h, _p(kp), _p(desc), F.N, *F.bounds, _p(has), n, *[_p(x) for x in q], float(th), self.mfNNratio, _p(out)))
        return nm, out[:F.N].copy()

    def SearchByProjectionLastFrame(self, CurrentFrame, valid, u, v, last_octave, last_angle, point_desc, point_has_obs,
                                    th, kp_has_point=None):
        """The matching loop of SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th,
        bMono=true) (src/ORBmatcher.cc:1355-1474) for given projections (u, v)."""
        ext = CurrentFrame.ext
        F = CurrentFrame
        kp, desc = _frame(F, "CurrentFrame")
        has = _mask(kp_has_point, F.N, "kp_has_point")
        n = len(valid)
        a = [_arr(valid, np.uint8, n, "valid"), _arr(u, np.float32, n, "u"), _arr(v, np.float32, n, "v"),
             _arr(last_octave, np.int32, n, "last_octave"), _arr(last_angle, np.float32, n, "last_angle"),
             _arr(point_desc, np.uint8, n, "point_desc", 32), _arr(point_has_obs, np.uint8, n, "point_has_obs")]
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_projection_frame(
            ext._h, _p(kp), _p(desc), F.N, *F.bounds, _p(has), n,
            *[_p(x) for x in a], float(th), int(self.mbCheckOrientation), _p(out)))
        return nm, out[:F.N].copy()

    def SearchByProjectionKeyFrame(self, CurrentFrame, valid, already_found, u, v, dist3d, min_distance, max_distance, kf_angle,
                                   point_desc, th, ORBdist, kp_has_point=None):
        """The matching loop of SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist)
        (src/ORBmatcher.cc:1476-1603; Tracking::Relocalization) for given projections (u, v) and depths: the bounds / depth
        tests, MapPoint::PredictScale, the window search and the rotation histogram run on the device.  min_distance /
        max_distance are the points' plain mfMinDistance / mfMaxDistance (the depth test forms 0.8f * min / 1.2f * max)."""
        ext = CurrentFrame.ext
        F = CurrentFrame
        kp, desc = _frame(F, "CurrentFrame")
        has = _mask(kp_has_point, F.N, "kp_has_point")
        n = len(valid)
        a = [_arr(valid, np.uint8, n, "valid"), _arr(already_found, np.uint8, n, "already_found"), _arr(u, np.float32, n, "u"),
             _arr(v, np.float32, n, "v"), _arr(dist3d, np.float32, n, "dist3d"), _arr(min_distance, np.float32, n, "min_distance"),
             _arr(max_distance, np.float32, n, "max_distance"), _arr(kf_angle, np.float32, n, "kf_angle"),
             _arr(point_desc, np.uint8, n, "point_desc", 32)]
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_projection_keyframe(
            ext._h, _p(kp), _p(desc), F.N, *F.bounds, _p(has), n, *[_p(x) for x in a],
            ext.log_scale_factor(), float(th), int(ORBdist), int(self.mbCheckOrientation), _p(out)))
        return nm, out[:F.N].copy()

    @staticmethod
    def _track_args(name, F, pose, table, idx, idx_name, lo, th, bounds, has_obs):
        """The checked inputs the three pose forms share: the frame, its bounds and pose, the table's Observations() > 0 flags
        (default: from the table's observation lists) and one index array into the table, every entry in [lo, table.n)."""
        kp, desc = _frame(F, name)
        bounds = F.bounds if bounds is None else bounds
        if len(bounds) != 4 or not (float(bounds[1]) > float(bounds[0]) and float(bounds[3]) > float(bounds[2])):
            raise ValueError("%s: bounds must be (min_x, max_x, min_y, max_y) with max > min" % name)
        if not float(th) > 0:
            raise ValueError("%s: th must be positive" % name)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        if len(idx) and (int(np.min(idx)) < lo or int(np.max(idx)) >= table.n):
            raise ValueError("%s: %s names a point outside the table (%d points)" % (name, idx_name, table.n))
        obs = (np.diff(table.obs_start) > 0).astype(np.uint8) if has_obs is None else _arr(has_obs, np.uint8, table.n, "point_has_obs")
        if table.n == 0:
            obs = np.zeros(1, np.uint8)
        P = np.ascontiguousarray(pose, KF_POSE_DTYPE).reshape(())
        return kp, desc, [float(b) for b in bounds], idx, obs, P

    def SearchLocalPoints(self, F, pose, kp_point, table, queries, query_seen=None, th=1.0, viewing_cos_limit=0.5, bounds=None,
                          point_has_obs=None):
        """Tracking::SearchLocalPoints (src/Tracking.cc:1134-1184) with Frame::isInFrustum (src/Frame.cc:273-329) and
        SearchByProjection(F, points, th) (src/ORBmatcher.cc:46-131) on the device.  pose: the frame's KF_POSE_DTYPE record;
        kp_point[i]: the table index of mvpMapPoints[i] or -1 (None = all -1); table: a MapPointTable; queries: mvpLocalMapPoints
        as distinct table indices; query_seen: see include/pgorb.h.  Returns a dict: nmatches, assigned, in_view, proj_x, proj_y,
        level, view_cos, kp_point_out, n_to_match."""
        name = "SearchLocalPoints"
        kp, desc, b, q, obs, P = self._track_args(name, F, pose, table, queries, "queries", 0, th, bounds, point_has_obs)
        nq = len(q)
        if len(np.unique(q)) != nq:
            raise ValueError("%s: a map point is queried twice" % name)
        slots = None if kp_point is None else _arr(kp_point, np.int32, F.N, "kp_point")
        if slots is not None:
            table.check_indices(slots, "kp_point", name)
        seen = None if query_seen is None else _arr(query_seen, np.uint8, nq, "query_seen")
        ext = F.ext
        m = max(nq, 1)
        iv, px, py = np.zeros(m, np.uint8), np.zeros(m, np.float32), np.zeros(m, np.float32)
        lv, vc = np.zeros(m, np.int32), np.zeros(m, np.float32)
        out, kpo, ntm = np.full(max(F.N, 1), -1, np.int32), np.full(max(F.N, 1), -1, np.int32), np.zeros(1, np.int32)
        t = table
        nm = ext._check(ext._L.pgorb_search_local_points(
            ext._h, _p(kp), _p(desc), F.N, *b, _p(P), None if slots is None else _p(slots), t.n, _p(t.points), _p(t.descriptors),
            _p(t.bad), _p(obs), nq, _p(q if nq else lv), None if seen is None else _p(seen), float(viewing_cos_limit), float(th),
            self.mfNNratio, _p(iv), _p(px), _p(py), _p(lv), _p(vc), _p(kpo), _p(ntm), _p(out)))
        return dict(nmatches=nm, assigned=out[:F.N].copy(), in_view=iv[:nq].copy(), proj_x=px[:nq].copy(), proj_y=py[:nq].copy(),
                    level=lv[:nq].copy(), view_cos=vc[:nq].copy(), kp_point_out=kpo[:F.N].copy(), n_to_match=int(ntm[0]))

    def SearchByProjectionLastFramePose(self, CurrentFrame, pose, last_keys, last_point, table, th, last_outlier=None,
                                        kp_has_point=None, bounds=None, point_has_obs=None):
        """All of SearchByProjection(CurrentFrame, LastFrame, th, bMono=true) (src/ORBmatcher.cc:1342-1474) on the device.
        last_keys: the last frame's keypoints (octave and angle are read); last_point[i]: the table index of
        LastFrame.mvpMapPoints[i] or -1; last_outlier: mvbOutlier (None = none).  Returns a dict: nmatches, assigned (last-frame
        keypoint indices), valid, u, v."""
        name = "SearchByProjectionLastFramePose"
        F = CurrentFrame
        kp, desc, b, lp, obs, P = self._track_args(name, F, pose, table, last_point, "last_point", -1, th, bounds, point_has_obs)
        nl = len(lp)
        lk = _arr(last_keys, KEYPOINT_DTYPE, nl, "last_keys")
        outl = None if last_outlier is None else _arr(last_outlier, np.uint8, nl, "last_outlier")
        has = None if kp_has_point is None else _arr(kp_has_point, np.uint8, F.N, "kp_has_point")
        ext = F.ext
        m = max(nl, 1)
        va, u, v = np.zeros(m, np.uint8), np.zeros(m, np.float32), np.zeros(m, np.float32)
        out = np.full(max(F.N, 1), -1, np.int32)
        t = table
        nm = ext._check(ext._L.pgorb_search_by_projection_last_frame(
            ext._h, _p(kp), _p(desc), F.N, *b, _p(P), None if has is None else _p(has), _p(lk if nl else out), nl,
            _p(lp if nl else out), None if outl is None else _p(outl), t.n, _p(t.points), _p(t.descriptors), _p(obs), float(th),
            int(self.mbCheckOrientation), _p(va), _p(u), _p(v), _p(out)))
        return dict(nmatches=nm, assigned=out[:F.N].copy(), valid=va[:nl].copy(), u=u[:nl].copy(), v=v[:nl].copy())

    def SearchByProjectionKeyFramePose(self, CurrentFrame, pose, kf_keys, kf_point, table, th, ORBdist, already_found=None,
                                       kp_has_point=None, bounds=None):
        """All of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1476-1603) on the device.
        kf_keys: pKF->mvKeysUn (the angle is read); kf_point[i]: the table index of GetMapPointMatches()[i] or -1;
        already_found: per key-frame keypoint (None = none).  Returns a dict: nmatches, assigned (key-frame keypoint indices), u,
        v, dist3d."""
        name = "SearchByProjectionKeyFramePose"
        F = CurrentFrame
        kp, desc, b, kfp, _, P = self._track_args(name, F, pose, table, kf_point, "kf_point", -1, th, bounds, None)
        nk = len(kfp)
        kk = _arr(kf_keys, KEYPOINT_DTYPE, nk, "kf_keys")
        found = None if already_found is None else _arr(already_found, np.uint8, nk, "already_found")
        has = None if kp_has_point is None else _arr(kp_has_point, np.uint8, F.N, "kp_has_point")
        ext = F.ext
        m = max(nk, 1)
        u, v, d3 = np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32)
        out = np.full(max(F.N, 1), -1, np.int32)
        t = table
        nm = ext._check(ext._L.pgorb_search_by_projection_keyframe_pose(
            ext._h, _p(kp), _p(desc), F.N, *b, _p(P), None if has is None else _p(has), _p(kk if nk else out), nk,
            _p(kfp if nk else out), None if found is None else _p(found), t.n, _p(t.points), _p(t.descriptors), _p(t.bad), float(th),
            int(ORBdist), int(self.mbCheckOrientation), _p(u), _p(v), _p(d3), _p(out)))
        return dict(nmatches=nm, assigned=out[:F.N].copy(), u=u[:nk].copy(), v=v[:nk].copy(), dist3d=d3[:nk].copy())

    def SearchByBoW(self, ext, kf_desc, kf_angle, kf_point_valid, kf_featvec, F, f_featvec):
        """SearchByBoW(KeyFrame* pKF, Frame &F, vpMapPointMatches) (src/ORBmatcher.cc:161-290).
        Feature vectors are the (nodes, starts, features) triples of ORBVocabulary.transform().
        Returns (nmatches, matches) with matches[j] = key-frame keypoint index or -1."""
        nkf = len(kf_angle)
        kd = _arr(kf_desc, np.uint8, nkf, "kf_desc", 32)
        ka = _arr(kf_angle, np.float32, nkf, "kf_angle")
        kv = _arr(kf_point_valid, np.uint8, nkf, "kf_point_valid")
        A, B = _featvec(kf_featvec, "kf_featvec"), _featvec(f_featvec, "f_featvec")
        fd = _arr(F.mDescriptors, np.uint8, F.N, "F descriptors", 32)
        fa = _arr(F.mvKeys["angle"], np.float32, F.N, "F angles")
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_bow(
            ext._h, _p(kd), _p(ka), _p(kv), nkf, _p(A[0]), _p(A[1]), _p(A[2]), len(A[0]),
            _p(fd), _p(fa), F.N, _p(B[0]), _p(B[1]), _p(B[2]), len(B[0]),
            self.mfNNratio, int(self.mbCheckOrientation), _p(out)))
        return nm, out[:F.N].copy()

    def SearchByBoWKeyFrames(self, ext, desc1, angle1, point_valid1, featvec1, desc2, angle2, point_valid2, featvec2):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:524-657).  Per key frame: descriptors, the angles
        of mvKeysUn, point_valid[i] = the keypoint has a map point that is not bad, and the FeatureVector as the (nodes, starts,
        features) triple of ORBVocabulary.transform().  Returns (nmatches, matches12) with matches12[i1] = the KF2 keypoint or -1."""
        n1, n2 = len(angle1), len(angle2)
        d1, d2 = _arr(desc1, np.uint8, n1, "desc1", 32), _arr(desc2, np.uint8, n2, "desc2", 32)
        a1, a2 = _arr(angle1, np.float32, n1, "angle1"), _arr(angle2, np.float32, n2, "angle2")
        v1, v2 = _arr(point_valid1, np.uint8, n1, "point_valid1"), _arr(point_valid2, np.uint8, n2, "point_valid2")
        A, B = _featvec(featvec1, "featvec1"), _featvec(featvec2, "featvec2")
        for fv, n, name in ((A, n1, "featvec1"), (B, n2, "featvec2")):
            m = int(fv[1][-1])
            if fv[1][0] != 0 or np.any(np.diff(fv[1]) < 0) or m > n or (m and int(fv[2][:m].max()) >= n) or np.any(np.diff(fv[0].astype(np.int64)) <= 0):
                raise ValueError("SearchByBoWKeyFrames: %s is not a FeatureVector of %d features (ascending nodes, rising starts)" % (name, n))
        out = np.full(max(n1, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_bow_keyframes(
            ext._h, _p(d1), _p(a1), _p(v1), n1, _p(A[0]), _p(A[1]), _p(A[2]), len(A[0]),
            _p(d2), _p(a2), _p(v2), n2, _p(B[0]), _p(B[1]), _p(B[2]), len(B[0]),
            self.mfNNratio, int(self.mbCheckOrientation), _p(out)))
        return nm, out[:n1].copy()

    def SearchForTriangulation(self, KF1, KF2, F12, epipole, fv1, fv2, has_point1=None, has_point2=None):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo=false) (src/ORBmatcher.cc:659-825, 142-159) on
        the undistorted keypoints of two Frames.  F12: 3x3 (or 9) float32, F12.at<float>(r, c) row-major; epipole = (ex, ey) in
        KF2; fv1 / fv2 the (nodes, starts, features) triples of ORBVocabulary.transform(); has_point*[i] = GetMapPoint(i) != NULL.
        Returns (nmatches, matches12) with matches12[i] = the KF2 keypoint matched to KF1 keypoint i, or -1 (vMatchedPairs =
        the (i, matches12[i]) with matches12[i] >= 0)."""
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        args = []
        for name, K, m, fv in (("KF1", KF1, has_point1, fv1), ("KF2", KF2, has_point2, fv2)):
            kp, desc = _frame(K, name)
            node, start, feat = _featvec(fv, name)
            args += [_p(kp), _p(desc), _p(_mask(m, K.N, name + " has_point")), K.N, _p(node), _p(start), _p(feat), len(node)]
        ext = KF1.ext
        m12 = np.full(max(KF1.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_for_triangulation(ext._h, *args, _p(F), float(np.float32(epipole[0])),
                                                              float(np.float32(epipole[1])), int(self.mbCheckOrientation), _p(m12)))
        return nm, m12[:KF1.N].copy()

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """(nmatches, vnMatches12); vbPrevMatched ([N1,2] float32) is updated in place, as in
        src/ORBmatcher.cc:407-522."""
        ext = F1.ext
        k1, d1 = _frame(F1, "F1")
        k2, d2 = _frame(F2, "F2")
        prev = _arr(vbPrevMatched, np.float32, F1.N, "vbPrevMatched", 2)
        m12 = np.full(max(F1.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_for_initialization(
            ext._h, _p(k1), _p(d1), F1.N, _p(k2), _p(d2), F2.N, *F2.bounds, _p(prev), _p(m12),
            int(windowSize), self.mfNNratio, int(self.mbCheckOrientation)))
        vbPrevMatched[...] = prev
        return nm, m12[:F1.N].copy()

    def Fuse(self, KF, pose, kf_id, kf_point, table, queries, th=3.0, bounds=None):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:827-979), monocular.  KF: a Frame-like object (ext, N,
        mvKeysUndistorted, mDescriptors; bounds = the Frame's (min_x, max_x, min_y, max_y), default KF.bounds); pose: a
        KF_POSE_DTYPE record; kf_id: KeyFrame::mnId; kf_point[i]: the table index of GetMapPoint(i) or -1 (None = all empty);
        table: a MapPointTable; queries[q]: the table index of vpMapPoints[q] or -1 for NULL.  Returns (nfused, action,
        best_idx, best_dist, kf_point_out) with action[q] one of FUSE_* (include/pgorb.h states how to replay them)."""
        ext = KF.ext
        kp, desc = _frame(KF, "KF")
        bounds = KF.bounds if bounds is None else bounds
        if len(bounds) != 4:
            raise ValueError("Fuse: bounds must be (min_x, max_x, min_y, max_y)")
        if not float(th) > 0:
            raise ValueError("Fuse: th must be positive")
        slots = np.full(max(KF.N, 1), -1, np.int32) if kf_point is None else _arr(kf_point, np.int32, KF.N, "kf_point")
        q = np.ascontiguousarray(queries, np.int32).reshape(-1)
        nq = len(q)
        table.check_indices(q, "queries")
        live = q[q >= 0]
        if len(np.unique(live)) != len(live):
            raise ValueError("Fuse: a map point is queried twice")
        occ = slots[:KF.N]
        table.check_indices(occ, "kf_point")
        occ = occ[occ >= 0]
        occ = occ[table.bad[occ] == 0]                     # a bad occupant only makes its queries FUSE_KF_POINT_BAD
        if len(np.unique(occ)) != len(occ):
            raise ValueError("Fuse: a point holds two slots of the key frame")
        st = table.obs_start
        owner = np.repeat(np.arange(table.n), np.diff(st))              # the point each observation belongs to
        listing = owner[table.obs_kf[:int(st[-1])] == np.uint64(kf_id)]
        if not np.all(np.isin(occ, listing)):
            raise ValueError("Fuse: the point in a slot does not list key frame %d" % int(kf_id))
        P = np.ascontiguousarray(pose, KF_POSE_DTYPE).reshape(())
        action = np.zeros(max(nq, 1), np.int32)
        bi = np.full(max(nq, 1), -1, np.int32)
        bd = np.full(max(nq, 1), -1, np.int32)
        out = np.full(max(KF.N, 1), -1, np.int32)
        t = table
        nf = ext._check(ext._L.pgorb_fuse(ext._h, _p(kp), _p(desc), KF.N, _p(P), int(kf_id), *[float(b) for b in bounds], _p(slots),
                                          t.n, _p(t.points), _p(t.descriptors), _p(t.bad), _p(t.obs_start), _p(t.obs_kf), nq,
                                          _p(q if nq else action), float(th), _p(action), _p(bi), _p(bd), _p(out)))
        return nf, action[:nq].copy(), bi[:nq].copy(), bd[:nq].copy(), out[:KF.N].copy()

    @staticmethod
    def _loop_args(name, KF, slots, table, queries, bounds):
        """The checked inputs FuseSim3 and SearchByProjectionSim3 share."""
        kp, desc = _frame(KF, "KF")
        bounds = KF.bounds if bounds is None else bounds
        if len(bounds) != 4:
            raise ValueError("%s: bounds must be (min_x, max_x, min_y, max_y)" % name)
        sl = np.full(max(KF.N, 1), -1, np.int32) if slots is None else _arr(slots, np.int32, KF.N, name + " slots")
        q = np.ascontiguousarray(queries, np.int32).reshape(-1)
        if len(q) and int(np.min(q)) < 0:
            raise ValueError("%s: a query is NULL or negative (the reference dereferences every point)" % name)
        table.check_indices(q, "queries", name)
        table.check_indices(sl[:KF.N], "slots", name)
        return kp, desc, [float(b) for b in bounds], sl, q

    def SearchBySim3(self, KF1, KF2, pose1, pose2, kf_point1, kf_point2, table, sim3, already1=None, already2=None, th=7.5,
                     bounds=None):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1106-1330), monocular.  KF1 /
        KF2: Frame-like objects; pose1 / pose2: KF_POSE_DTYPE records (GetRotation() | GetTranslation(); both projections use
        pose1's camera); kf_point1 / 2: table indices of the slots' points or -1 (None = none); table: a MapPointTable; sim3: a
        SIM3_DTYPE record (sim3_record()); already1 / 2: vbAlreadyMatched1 / 2 (None = none).  Returns (nFound, match12) with
        match12[i1] = the KF2 keypoint of every newly found pair, or -1."""
        name = "SearchBySim3"
        if not float(th) > 0:
            raise ValueError("SearchBySim3: th must be positive")
        k1, d1 = _frame(KF1, "KF1")
        k2, d2 = _frame(KF2, "KF2")
        bounds = KF1.bounds if bounds is None else bounds
        if len(bounds) != 4:
            raise ValueError("SearchBySim3: bounds must be (min_x, max_x, min_y, max_y)")
        s1 = np.full(max(KF1.N, 1), -1, np.int32) if kf_point1 is None else _arr(kf_point1, np.int32, KF1.N, "kf_point1")
        s2 = np.full(max(KF2.N, 1), -1, np.int32) if kf_point2 is None else _arr(kf_point2, np.int32, KF2.N, "kf_point2")
        table.check_indices(s1[:KF1.N], "kf_point1", name)
        table.check_indices(s2[:KF2.N], "kf_point2", name)
        a1, a2 = _mask(already1, KF1.N, "already1"), _mask(already2, KF2.N, "already2")
        X = np.ascontiguousarray(sim3, SIM3_DTYPE)
        if X.size != 1:
            raise ValueError("SearchBySim3: sim3 must be one SIM3_DTYPE record")
        P1, P2 = (np.ascontiguousarray(P, KF_POSE_DTYPE).reshape(()) for P in (pose1, pose2))
        ext, t = KF1.ext, table
        m12 = np.full(max(KF1.N, 1), -1, np.int32)
        nf = ext._check(ext._L.pgorb_search_by_sim3(ext._h, _p(k1), _p(d1), KF1.N, _p(P1), _p(s1), _p(a1), _p(k2), _p(d2), KF2.N, _p(P2),
                                                    _p(s2), _p(a2), *[float(b) for b in bounds], t.n, _p(t.points), _p(t.descriptors),
                                                    _p(t.bad), _p(X), float(th), _p(m12)))
        return nf, m12[:KF1.N].copy()

    def SearchByProjectionSim3(self, KF, scw_pose, matched_in, table, queries, th=10, bounds=None):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:292-405), monocular.  KF: a
        Frame-like object; scw_pose: the decomposed Scw as a KF_POSE_DTYPE record (sim3_pose()); matched_in[i]: the table index
        of vpMatched[i] or -1 (None = all -1); table: a MapPointTable (observations unused); queries: table indices, repeats
        allowed; th: an int.  Returns (nmatches, assigned, matched_out): assigned[i] = the query written into vpMatched[i]."""
        if int(th) != th or int(th) < 1:
            raise ValueError("SearchByProjectionSim3: th must be a positive int")
        kp, desc, b, sl, q = self._loop_args("SearchByProjectionSim3", KF, matched_in, table, queries, bounds)
        ext, t, nq = KF.ext, table, len(q)
        P = np.ascontiguousarray(scw_pose, KF_POSE_DTYPE).reshape(())
        asg = np.full(max(KF.N, 1), -1, np.int32)
        out = np.full(max(KF.N, 1), -1, np.int32)
        nm = ext._check(ext._L.pgorb_search_by_projection_sim3(ext._h, _p(kp), _p(desc), KF.N, _p(P), *b, _p(sl), t.n, _p(t.points),
                                                               _p(t.descriptors), _p(t.bad), nq, _p(q if nq else asg), int(th),
                                                               _p(asg), _p(out)))
        return nm, asg[:KF.N].copy(), out[:KF.N].copy()

    def FuseSim3(self, KF, scw_pose, kf_point, table, queries, th=4.0, bounds=None):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:981-1104), monocular.  Arguments as
        SearchByProjectionSim3's, with kf_point[i] = the table index of GetMapPoint(i) or -1.  Returns (nfused, action,
        replace_point, best_idx, best_dist, kf_point_out); action[q] is FUSE_SKIPPED, FUSE_NO_MATCH, FUSE_ADDED,
        FUSE_KF_POINT_BAD or FUSE_REPLACE_REQUESTED, the last with replace_point[q] = the table index of vpReplacePoint[q]."""
        if not float(th) > 0:
            raise ValueError("FuseSim3: th must be positive")
        kp, desc, b, sl, q = self._loop_args("FuseSim3", KF, kf_point, table, queries, bounds)
        ext, t, nq = KF.ext, table, len(q)
        P = np.ascontiguousarray(scw_pose, KF_POSE_DTYPE).reshape(())
        action = np.zeros(max(nq, 1), np.int32)
        rep, bi, bd = (np.full(max(nq, 1), -1, np.int32) for _ in range(3))
        out = np.full(max(KF.N, 1), -1, np.int32)
        nf = ext._check(ext._L.pgorb_fuse_sim3(ext._h, _p(kp), _p(desc), KF.N, _p(P), *b, _p(sl), t.n, _p(t.points), _p(t.descriptors),
                                               _p(t.bad), nq, _p(q if nq else action), float(th), _p(action), _p(rep), _p(bi), _p(bd),
                                               _p(out)))
        return nf, action[:nq].copy(), rep[:nq].copy(), bi[:nq].copy(), bd[:nq].copy(), out[:KF.N].copy()

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else a
        b = np.frombuffer(bytes(b), np.uint8) if isinstance(b, (bytes, bytearray)) else b
        a = np.ascontiguousarray(a, np.uint8).reshape(32)
        b = np.ascontiguousarray(b, np.uint8).reshape(32)
        return _lib.lib().pgorb_descriptor_distance(_p(a), _p(b))


# pgorb_kf_pose: a key frame's GetPose() rows 0-2 ([R | t] row-major), GetCameraCenter() and camera (include/pgorb.h)
KF_POSE_DTYPE = _lib.KF_POSE_DTYPE
# pgorb_new_map_point: one point of CreateNewMapPoints
NEW_MAP_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                                ("min_distance", "<f4"), ("max_distance", "<f4")])
CNM_SKIPPED = -1                 # count[s] of a neighbour the baseline test skipped
CNM_MAX_NEIGHBOURS = 64


# pgorb_map_point: what ORBmatcher::Fuse reads of a MapPoint's pose fields (the plain mfMin/MaxDistance, not the getters)
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4")])
# action codes of ORBmatcher.Fuse (include/pgorb.h)
FUSE_SKIPPED, FUSE_NO_MATCH, FUSE_ADDED, FUSE_MERGED_INTO_KF_POINT, FUSE_REPLACED_KF_POINT, FUSE_KF_POINT_BAD = range(6)
FUSE_REPLACE_REQUESTED = 6       # ORBmatcher.FuseSim3 only: vpReplacePoint[q] = the slot's occupant


class MapPointTable:
    """The map points one Fuse call reads, shared by its queries and the key frame's slots: points (MAP_POINT_DTYPE),
    descriptors [n, 32], bad flags (None = none bad) and observations as CSR: obs_kf[obs_start[i]:obs_start[i + 1]] = the
    KeyFrame::mnId of every key frame observing point i, ascending and without repeats."""

    def __init__(self, points, descriptors, bad, obs_start, obs_kf):
        self.points = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
        n = self.n = len(self.points)
        self.descriptors = _arr(descriptors, np.uint8, n, "point descriptors", 32)
        self.bad = _mask(bad, n, "point bad")
        self.obs_start = _arr(obs_start, np.int32, n + 1, "obs_start")
        self.obs_kf = np.ascontiguousarray(obs_kf, np.uint64).reshape(-1)
        st = self.obs_start
        if st[0] != 0 or np.any(np.diff(st) < 0) or len(self.obs_kf) < int(st[-1]):
            raise ValueError("MapPointTable: obs_start must rise from 0 to at most len(obs_kf)")
        k = self.obs_kf[:int(st[-1])]
        inner = np.ones(len(k), bool)
        inner[st[:-1][st[:-1] < len(k)]] = False           # the first entry of each list has no predecessor in it
        if len(k) > 1 and np.any(inner[1:] & (k[1:] <= k[:-1])):
            raise ValueError("MapPointTable: an observation list is unsorted or repeats a key frame")
        if len(self.obs_kf) == 0:
            self.obs_kf = np.zeros(1, np.uint64)

    def check_indices(self, idx, name, routine="Fuse"):
        if len(idx) and (int(np.min(idx)) < -1 or int(np.max(idx)) >= self.n):
            raise ValueError("%s: %s names a point outside the table (%d points)" % (routine, name, self.n))


def kf_pose(Tcw, Ow, fx, fy, cx, cy, invfx=None, invfy=None):
    """A KF_POSE_DTYPE record; invfx / invfy default to 1.0f/fx, 1.0f/fy (Frame.cc:135-136 computes them in float)."""
    r = np.zeros((), KF_POSE_DTYPE)
    r["Tcw"] = np.asarray(Tcw, np.float32).reshape(3, 4).reshape(12)
    r["Ow"] = np.asarray(Ow, np.float32).reshape(3)
    fx, fy = np.float32(fx), np.float32(fy)
    r["fx"], r["fy"], r["cx"], r["cy"] = fx, fy, np.float32(cx), np.float32(cy)
    r["invfx"] = np.float32(1.0) / fx if invfx is None else np.float32(invfx)
    r["invfy"] = np.float32(1.0) / fy if invfy is None else np.float32(invfy)
    return r


# pgorb_sim3: SearchBySim3's transform as the caller's cv::Mat arithmetic produced it (ORBmatcher.cc:1123-1125)
SIM3_DTYPE = np.dtype([("sR12", "<f4", (9,)), ("t12", "<f4", (3,)), ("sR21", "<f4", (9,)), ("t21", "<f4", (3,))])


# pgorb_sim3_params / pgorb_sim3_estimate: Sim3Solver's parameter block and one (R12, t12, s12) (include/pgorb.h)
SIM3_PARAMS_DTYPE = np.dtype([("probability", "<f4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("fix_scale", "<i4"),
                              ("first_iteration", "<i4"), ("niterations", "<i4"), ("best_inliers_in", "<i4")])
SIM3_ESTIMATE_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4")])
S3_FEW, S3_FOUND, S3_NO_MORE, S3_INFO, SIM3_MAX_ITERATIONS = 1, 2, 4, 8, 1024


def sim3_record(sR12, t12, sR21, t21):
    """A SIM3_DTYPE record of sR12 = s12*R12, t12, sR21 = (1.0/s12)*R12.t() and t21 = -sR21*t12, each as the caller computed it."""
    r = np.zeros((), SIM3_DTYPE)
    r["sR12"], r["sR21"] = np.asarray(sR12, np.float32).reshape(9), np.asarray(sR21, np.float32).reshape(9)
    r["t12"], r["t21"] = np.asarray(t12, np.float32).reshape(3), np.asarray(t21, np.float32).reshape(3)
    return r


def sim3_pose(Scw, fx, fy, cx, cy):
    """The KF_POSE_DTYPE record of a 4x4 (or 3x4) float Scw as ORBmatcher.cc:301-305 / :990-994 decompose it:
        scw = sqrt(sRcw.row(0).dot(sRcw.row(0)));  Rcw = sRcw/scw;  tcw = Scw.rowRange(0,3).col(3)/scw;  Ow = -Rcw.t()*tcw
    under the project's cv::Mat readings.  RECALLED, not checked against an OpenCV build: Mat::dot sums
    in double and scw is its double sqrt rounded to float; Mat / double is the scaled copy Mat * (1/scw) with the factor 1.0/scw
    formed in double and applied in float; -Rcw.t()*tcw is gemm's small-matrix path, float sums, then times alpha = -1 in
    double."""
    S = np.asarray(Scw, np.float32)
    if S.shape not in ((4, 4), (3, 4)):
        raise ValueError("sim3_pose: Scw must be 4x4 or 3x4")
    f32, f64 = np.float32, np.float64
    r0 = S[0, :3].astype(f64)
    scw = f32(np.sqrt(f64(r0[0] * r0[0]) + f64(r0[1] * r0[1]) + f64(r0[2] * r0[2])))
    if not scw > 0:
        raise ValueError("sim3_pose: Scw has no scale")
    a = f32(f64(1.0) / f64(scw))
    R = (S[:3, :3] * a).astype(f32)
    t = (S[:3, 3] * a).astype(f32)
    Ow = [f32(f64(f32(f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1])) + f32(R[2, i] * t[2]))) * f64(-1.0)) for i in range(3)]
    return kf_pose(np.concatenate([R, t.reshape(3, 1)], 1), Ow, fx, fy, cx, cy)


# pgorb_pose_optimization: the status bits and the length of its info record (include/pgorb.h)
PO_FEW, PO_NONFINITE, PO_INFO = 1, 2, 8
# pgorb_optimize_sim3: the same
OS3_FEW, OS3_NONFINITE, OS3_INFO = 1, 2, 8
# pgorb_local_bundle_adjustment: status bits, the info record, the roles and the capacities of one window
LBA_NOTHING, LBA_NONFINITE, LBA_LIMIT, LBA_INFO = 1, 2, 4, 10
LBA_ROLE_NONE, LBA_ROLE_LOCAL, LBA_ROLE_FIXED = 0, 1, 2
LBA_MAX_LOCAL_KF, LBA_MAX_FIXED_KF, LBA_MAX_POINTS, LBA_MAX_EDGES = 64, 256, 8192, 65536
EG_NOTHING, EG_NONFINITE, EG_LIMIT, EG_INFO = 1, 2, 4, 10
EG_MAX_KF, EG_MAX_EDGES, EG_MAX_ENVELOPE_BLOCKS = 2048, 65536, 131072
GBA_NOTHING, GBA_NONFINITE, GBA_LIMIT, GBA_INFO = 1, 2, 4, 8
GBA_MAX_KF, GBA_MAX_POINTS, GBA_MAX_EDGES, GBA_MAX_ENVELOPE_BLOCKS = 2048, 262144, 2097152, 131072
SIM3D_DTYPE = np.dtype([("r", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])                    # pgorb_sim3d: g2o::Sim3
EG_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<i4"), ("pad", "<i4"), ("chi2", "<f8")])


class Optimizer:
    """Optimizer::PoseOptimization (thirdparty/orb-slam2/src/Optimizer.cc:239-451, monocular), Optimizer::OptimizeSim3
    (:1046-1241), Optimizer::LocalBundleAdjustment (:453-778) and Optimizer::OptimizeEssentialGraph (:781-1044) on the GPU."""

    @staticmethod
    def PoseOptimization(frame_keys, pose, kp_point, table, discard_outliers=False, point_has_obs=None):
        """frame_keys: a Frame-like object (ext, N, mvKeysUndistorted: pt and octave are read); pose: the frame's KF_POSE_DTYPE
        record (Tcw and the camera are read); kp_point[i]: the table index of mvpMapPoints[i] or -1; table: a MapPointTable (pos is
        read; point_has_obs defaults to its observation lists).  discard_outliers: run the loop of Tracking.cc:768-787 too.  Every
        input the library's checked call refuses is a ValueError here, before the library is called.  Returns a dict: ret (the
        reference's return value), pose (a complete KF_POSE_DTYPE record), outlier, kp_point_out, nmatches_map, chi2, status
        (PO_FEW | PO_NONFINITE bits), rounds, iterations (of rounds 0..3), trials, edges."""
        name = "PoseOptimization"
        F = frame_keys
        n = int(F.N)
        if n < 0:
            raise ValueError("%s: a negative keypoint count" % name)
        kp = _arr(F.mvKeysUndistorted, KEYPOINT_DTYPE, n, name + " keypoints")
        slots = _arr(kp_point, np.int32, n, "kp_point")
        table.check_indices(slots, "kp_point", name)
        P = np.ascontiguousarray(pose, KF_POSE_DTYPE).reshape(())
        cam = [float(P[k]) for k in ("fx", "fy", "cx", "cy")]
        if not (np.isfinite(P["Tcw"]).all() and np.isfinite(cam).all()):
            raise ValueError("%s: the pose or the camera is not finite" % name)
        if cam[0] == 0.0 or cam[1] == 0.0:
            raise ValueError("%s: fx or fy is zero" % name)
        held = slots >= 0
        if held.any() and not np.isfinite(table.points["pos"][slots[held]]).all():
            raise ValueError("%s: a referenced point is not finite" % name)
        obs = (np.diff(table.obs_start) > 0).astype(np.uint8) if point_has_obs is None else _arr(point_has_obs, np.uint8, table.n, "point_has_obs")
        if table.n == 0:
            obs = np.zeros(1, np.uint8)
        ext = F.ext
        levels = ext.GetLevels()
        if held.any() and (int(kp["octave"][held].min()) < 0 or int(kp["octave"][held].max()) >= levels):
            raise ValueError("%s: an octave is outside the extractor's %d levels" % (name, levels))
        m = max(n, 1)
        out = np.zeros((), KF_POSE_DTYPE)
        fl, ko, chi = np.zeros(m, np.uint8), np.full(m, -1, np.int32), np.zeros(m, np.float32)
        nmap, info = np.zeros(1, np.int32), np.zeros(PO_INFO, np.int32)
        ret = ext._check(ext._L.pgorb_pose_optimization(
            ext._h, _p(kp if n else chi), n, _p(P), _p(slots if n else ko), table.n, _p(table.points), _p(obs), int(bool(discard_outliers)),
            _p(out), _p(fl), _p(ko), _p(nmap), _p(chi), _p(info)))
        return dict(ret=ret, pose=out, outlier=fl[:n].copy(), kp_point_out=ko[:n].copy(), nmatches_map=int(nmap[0]), chi2=chi[:n].copy(),
                    status=int(info[0]), rounds=int(info[1]), iterations=[int(x) for x in info[2:6]], trials=int(info[6]), edges=int(info[7]))


    @staticmethod
    def check_sim3(name, KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, new_matches12, table, estimate, th2):
        """pgorb_optimize_sim3's checks, without a device; returns the arrays the library reads."""
        n1, n2 = int(KF1.N), int(KF2.N)
        if n1 < 0 or n2 < 0:
            raise ValueError("%s: a negative keypoint count" % name)
        m = _arr(matches12, np.int32, n1, "matches12")
        nm = None if new_matches12 is None else _arr(new_matches12, np.int32, n1, "new_matches12")
        for nme, a in (("matches12", m), ("new_matches12", nm)):
            if a is not None and n1 and (int(a.min()) < -1 or int(a.max()) >= n2):
                raise ValueError("%s: %s is outside [-1, n2)" % (name, nme))
        e = np.ascontiguousarray(estimate, SIM3_ESTIMATE_DTYPE).reshape(())
        if not (np.isfinite(e["R12"]).all() and np.isfinite(e["t12"]).all() and np.isfinite(e["s12"])):
            raise ValueError("%s: the estimate is not finite" % name)
        if not float(e["s12"]) > 0.0:
            raise ValueError("%s: the estimate's scale is not positive" % name)
        if not (float(np.float32(th2)) > 0.0 and np.isfinite(np.float32(th2))):
            raise ValueError("%s: th2 is not positive" % name)
        merged = m if nm is None else np.where(nm >= 0, nm, m).astype(np.int32)
        a = Sim3Solver.check(name, KF1, KF2, pose1, pose2, kf_point1, kf_point2, merged, table)
        a["m"], a["nm"], a["e"] = m, nm, e
        return a

    @staticmethod
    def OptimizeSim3(KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, table, estimate, th2=10.0, bFixScale=False, new_matches12=None):
        """Optimizer::OptimizeSim3 (thirdparty/orb-slam2/src/Optimizer.cc:1046-1241) on the GPU: step 4 of LoopClosing::ComputeSim3.
        The key frames, poses, slots and the table as for Sim3Solver; matches12[i1] = the KF2 keypoint or -1 (the solver's
        matches12_out); new_matches12 (or None) = what SearchBySim3 wrote, replacing an entry where it is >= 0; estimate = a
        SIM3_ESTIMATE_DTYPE record (R12, t12, s12: the solver's `found`).  Every input the library's checked call refuses is a
        ValueError here, before the library is called.  Returns a dict: ret (nIn), estimate (SIM3_ESTIMATE_DTYPE), matches12_out,
        chi2_12, chi2_21, scw_pose (a complete KF_POSE_DTYPE record for SearchByProjectionSim3; zeroed with a status), status
        (OS3_FEW | OS3_NONFINITE bits), correspondences, nbad, iterations and trials (of the two optimize calls), more_iterations."""
        a = Optimizer.check_sim3("OptimizeSim3", KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, new_matches12, table, estimate, th2)
        ext, t = KF1.ext, table
        n1, n2 = a["n1"], a["n2"]
        eo, sp = np.zeros((), SIM3_ESTIMATE_DTYPE), np.zeros((), KF_POSE_DTYPE)
        mo, c12, c21 = np.full(max(n1, 1), -1, np.int32), np.zeros(max(n1, 1), np.float32), np.zeros(max(n1, 1), np.float32)
        info = np.zeros(OS3_INFO, np.int32)
        pad = lambda x, n, dt: x if n else np.zeros(1, dt)
        ret = ext._check(ext._L.pgorb_optimize_sim3(
            ext._h, _p(pad(a["k1"], n1, KEYPOINT_DTYPE)), n1, _p(a["P1"]), _p(pad(a["s1"], n1, np.int32)), _p(pad(a["k2"], n2, KEYPOINT_DTYPE)), n2,
            _p(a["P2"]), _p(pad(a["s2"], n2, np.int32)), _p(pad(a["m"], n1, np.int32)), None if a["nm"] is None else _p(pad(a["nm"], n1, np.int32)),
            t.n, _p(t.points), _p(t.bad), _p(a["e"]), float(np.float32(th2)), int(bool(bFixScale)), _p(eo), _p(mo), _p(c12), _p(c21), _p(sp), _p(info)))
        return dict(ret=ret, estimate=eo, matches12_out=mo[:n1].copy(), chi2_12=c12[:n1].copy(), chi2_21=c21[:n1].copy(), scw_pose=sp,
                    status=int(info[0]), correspondences=int(info[1]), nbad=int(info[2]), iterations=[int(info[3]), int(info[5])],
                    trials=[int(info[4]), int(info[6])], more_iterations=int(info[7]))

    @staticmethod
    def OptimizeSim3_batch_device(ext, d_kps, d_n, cap_per_frame, d_pair_kf1, d_pair_kf2, d_pose, d_kf_point, d_matches12, npoints, d_points,
                                  d_point_bad, d_estimate, th2=10.0, bFixScale=False, d_new_matches12=None, stream=None):
        """pgorb_optimize_sim3_batch_device over resident torch tensors: pair p refines key frames d_pair_kf1[p] and d_pair_kf2[p]
        from d_estimate[p] (the bytes of SIM3_ESTIMATE_DTYPE per pair: Sim3Solver.iterate_batch_device's `found`); d_matches12 and
        d_new_matches12 (or None) are [npairs][cap].  th2, the sizes and the tensors' element types are checked here; the arrays'
        contents are not read: the batched form counts a bad index as no correspondence.  Returns a dict of freshly allocated
        tensors: estimate, scw_pose (bytes of their dtypes per pair), matches12_out, chi2_12, chi2_21 [npairs][cap],
        info [npairs][OS3_INFO], nin [npairs]."""
        import torch
        name = "Optimizer.OptimizeSim3_batch_device"
        if not (float(np.float32(th2)) > 0.0 and np.isfinite(np.float32(th2))):
            raise ValueError("%s: th2 is not positive" % name)
        for nm, t_ in (("d_pair_kf1", d_pair_kf1), ("d_pair_kf2", d_pair_kf2), ("d_matches12", d_matches12), ("d_n", d_n), ("d_kf_point", d_kf_point),
                       ("d_new_matches12", d_new_matches12)):
            if t_ is not None and t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the pair count and the row lengths are taken from element counts)" % (name, nm))
        npairs, cap = int(d_pair_kf1.numel()), int(cap_per_frame)
        if cap < 1 or cap > Sim3Solver.MAX_N:
            raise ValueError("%s: cap_per_frame outside [1, %d]" % (name, Sim3Solver.MAX_N))
        if int(d_pair_kf2.numel()) != npairs or int(npoints) < 0:
            raise ValueError("%s: the pair lists differ in length or npoints is negative" % name)
        if d_matches12.numel() != npairs * cap or (d_new_matches12 is not None and d_new_matches12.numel() != npairs * cap):
            raise ValueError("%s: d_matches12 and d_new_matches12 must be [npairs][cap]" % name)
        if d_estimate.numel() * d_estimate.element_size() != npairs * SIM3_ESTIMATE_DTYPE.itemsize:
            raise ValueError("%s: d_estimate must hold one estimate per pair" % name)
        nframes = int(d_n.numel())
        if d_kf_point.numel() != nframes * cap or d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_pose.numel() * d_pose.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps, d_kf_point and d_pose must hold one row per frame of d_n" % name)
        if d_points.numel() * d_points.element_size() < int(npoints) * MAP_POINT_DTYPE.itemsize or \
                (d_point_bad is not None and d_point_bad.numel() * d_point_bad.element_size() < int(npoints)):
            raise ValueError("%s: the table is shorter than npoints" % name)
        L, h = ext._L, ext._h
        dev = d_matches12.device
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(estimate=e((npairs, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8), scw_pose=e((npairs, KF_POSE_DTYPE.itemsize), torch.uint8),
                   matches12_out=e((npairs, cap), torch.int32), chi2_12=e((npairs, cap), torch.float32), chi2_21=e((npairs, cap), torch.float32),
                   info=e((npairs, OS3_INFO), torch.int32), nin=e((npairs,), torch.int32))
        q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(L.pgorb_optimize_sim3_batch_device(
            h, q(d_kps), q(d_n), cap, q(d_pair_kf1), q(d_pair_kf2), npairs, q(d_pose), q(d_kf_point), q(d_matches12), q(d_new_matches12),
            int(npoints), q(d_points), q(d_point_bad), q(d_estimate), float(np.float32(th2)), int(bool(bFixScale)), q(out["estimate"]),
            q(out["matches12_out"]), q(out["chi2_12"]), q(out["chi2_21"]), q(out["scw_pose"]), q(out["info"]), q(out["nin"]), C.c_void_p(s)))
        return out

    @staticmethod
    def LocalBundleAdjustment(key_frames, poses, kf_point, local_kf, points, obs_start, obs_frame, obs_idx, point_bad=None, kf_bad=None,
                              kf_fixed_id0=None, rounds=2, ext=None):
        """Optimizer::LocalBundleAdjustment (thirdparty/orb-slam2/src/Optimizer.cc:453-778, monocular) on the GPU.  key_frames:
        Frame-like objects (ext, N, mvKeysUndistorted: pt and octave are read); poses[f]: KF_POSE_DTYPE (Tcw and the camera are
        read); kf_point[f][i] = the table index of GetMapPoint(i) or -1; kf_bad[f] = isBad(), kf_fixed_id0[f] = (mnId == 0) (None =
        none); local_kf: pKF and its covisible key frames as positions in key_frames, in any order.  points (MAP_POINT_DTYPE; pos is
        read), point_bad, and the observations as CSR of (obs_frame, obs_idx) as for RefreshMapPoints.  rounds: 2, or 1 for
        bDoMore == false.  Every input pgorb_local_bundle_adjustment refuses is a ValueError here, before the library is called;
        a window past a capacity (LBA_MAX_*) raises PgorbError.  Returns a dict: ret (the erased observations), poses (a copy with
        the local key frames replaced), points (a copy with the local points' pos replaced), erase / chi2 / level per observation,
        to_erase = vToErase as (frame, point) pairs in CSR order, is_local, role, status, edges, local_points, local_kfs, fixed_kfs,
        iterations and trials (of the two optimize calls), level1."""
        fn = "LocalBundleAdjustment"
        nkf = len(key_frames)
        if ext is None:
            if not nkf:
                raise ValueError(fn + ": no key frame and no ext")
            ext = key_frames[0].ext
        if rounds not in (1, 2):
            raise ValueError(fn + ": rounds must be 1 or 2")
        if len(poses) != nkf or len(kf_point) != nkf:
            raise ValueError(fn + ": key_frames, poses and kf_point differ in length")
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))       # a copy: moved in place
        n = len(pts)
        if not np.isfinite(pts["pos"]).all():
            raise ValueError(fn + ": a point is not finite")
        levels = ext.GetLevels()
        P = np.zeros(max(nkf, 1), KF_POSE_DTYPE)
        keep = []
        kps, slots = [(C.c_void_p * max(nkf, 1))() for _ in range(2)]
        nk = np.zeros(max(nkf, 1), np.int32)
        octs = []
        for f, K in enumerate(key_frames):
            if int(K.N) < 0:
                raise ValueError("%s: key frame %d has a negative keypoint count" % (fn, f))
            kp = _arr(K.mvKeysUndistorted, KEYPOINT_DTYPE, K.N, "key frame %d keypoints" % f)
            sl = _arr(kf_point[f], np.int32, K.N, "kf_point[%d]" % f)
            if K.N and (int(sl.min()) < -1 or int(sl.max()) >= n):
                raise ValueError("%s: a slot's point index is out of range" % fn)
            kp_buf, sl_buf = (kp, sl) if K.N else (np.zeros(1, KEYPOINT_DTYPE), np.zeros(1, np.int32))
            keep += [kp_buf, sl_buf]
            kps[f], slots[f], nk[f] = kp_buf.ctypes.data, sl_buf.ctypes.data, K.N
            octs.append(kp["octave"])
            P[f] = np.asarray(poses[f], KF_POSE_DTYPE).reshape(())
            cam = [float(P[f][k]) for k in ("fx", "fy", "cx", "cy")]
            if not (np.isfinite(P[f]["Tcw"]).all() and np.isfinite(cam).all()):
                raise ValueError(fn + ": a pose or a camera is not finite")
            if cam[0] == 0.0 or cam[1] == 0.0:
                raise ValueError(fn + ": fx or fy is zero")
        kb, i0, pb = _mask(kf_bad, nkf, "kf_bad"), _mask(kf_fixed_id0, nkf, "kf_fixed_id0"), _mask(point_bad, n, "point_bad")
        lk = np.ascontiguousarray(local_kf, np.int32).reshape(-1)
        if len(lk) and (int(lk.min()) < 0 or int(lk.max()) >= nkf):
            raise ValueError(fn + ": a local key frame is out of range")
        st = _arr(obs_start, np.int32, n + 1, "obs_start")
        of = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
        oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
        if st[0] != 0 or np.any(np.diff(st) < 0) or len(of) < int(st[-1]) or len(oi) < int(st[-1]):
            raise ValueError(fn + ": obs_start must rise from 0 to at most len(obs_frame), len(obs_idx)")
        m = int(st[-1])
        if m and (of[:m].min() < 0 or of[:m].max() >= nkf or oi[:m].min() < 0 or np.any(oi[:m] >= nk[np.clip(of[:m], 0, max(nkf - 1, 0))])):
            raise ValueError(fn + ": an observation names a key frame or keypoint out of range")
        owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(st))
        if len(np.unique(owner * max(nkf, 1) + of[:m])) != m:
            raise ValueError(fn + ": a list names a key frame twice")
        for k in range(m):
            o = int(octs[of[k]][oi[k]])
            if o < 0 or o >= levels:
                raise ValueError("%s: an octave is outside the extractor's %d levels" % (fn, levels))
        if len(of) == 0:
            of, oi = np.zeros(1, np.int32), np.zeros(1, np.int32)
        po = np.zeros(max(nkf, 1), KF_POSE_DTYPE)
        er, lv, chi = np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.float32)
        il, ro, info = np.zeros(max(n, 1), np.uint8), np.zeros(max(nkf, 1), np.uint8), np.zeros(LBA_INFO, np.int32)
        pts_buf = pts if n else np.zeros(1, MAP_POINT_DTYPE)
        ret = ext._check(ext._L.pgorb_local_bundle_adjustment(
            ext._h, nkf, kps, _p(nk), _p(P), _p(kb), slots, _p(i0), len(lk), _p(lk if len(lk) else np.zeros(1, np.int32)), n, _p(pts_buf), _p(pb),
            _p(st), _p(of), _p(oi), int(rounds), _p(po), _p(er), _p(chi), _p(lv), _p(il), _p(ro), _p(info)))
        er = er[:m].copy()
        return dict(ret=ret, poses=po[:nkf].copy(), points=pts, erase=er, chi2=chi[:m].copy(), level=lv[:m].copy(),
                    to_erase=[(int(of[k]), int(owner[k])) for k in np.flatnonzero(er)], is_local=il[:n].copy(), role=ro[:nkf].copy(),
                    status=int(info[0]), edges=int(info[1]), local_points=int(info[2]), local_kfs=int(info[3]), fixed_kfs=int(info[4]),
                    iterations=[int(info[5]), int(info[7])], trials=[int(info[6]), int(info[8])], level1=int(info[9]))

    @staticmethod
    def LocalBundleAdjustment_batch_device(ext, d_kps, d_n, cap_per_frame, d_pose, d_kf_point, d_win_start, d_win_kf, npoints, d_points,
                                           d_obs_start, d_obs_frame, d_obs_idx, d_point_bad=None, d_kf_bad=None, d_kf_fixed_id0=None,
                                           rounds=2, d_pose_out=None, stream=None):
        """pgorb_local_bundle_adjustment_batch_device over resident torch tensors: window w adjusts the key frames
        d_win_kf[d_win_start[w] : d_win_start[w + 1]] of one batch and the points they hold, IN PLACE in d_points.  Two windows of one
        call must not share a local point (include/pgorb.h); nothing checks it.  The sizes and element types are checked here; the
        contents are not read.  d_pose_out (bytes of KF_POSE_DTYPE per frame; default: a copy of d_pose) is written for the local key
        frames only.  Returns a dict of tensors: pose_out, erase / chi2 / level [nwin][nobs], is_local [nwin][npoints], role
        [nwin][nframes], info [nwin][LBA_INFO], nerased [nwin].  The chain into pMP->UpdateNormalAndDepth() is
        pgorb_refresh_map_points_batch_device on the same d_points with d_pose = pose_out and select = the local points."""
        import torch
        name = "Optimizer.LocalBundleAdjustment_batch_device"
        if rounds not in (1, 2):
            raise ValueError(name + ": rounds must be 1 or 2")
        for nm, t_ in (("d_n", d_n), ("d_kf_point", d_kf_point), ("d_win_start", d_win_start), ("d_win_kf", d_win_kf), ("d_obs_start", d_obs_start),
                       ("d_obs_frame", d_obs_frame), ("d_obs_idx", d_obs_idx)):
            if t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the counts are taken from element counts)" % (name, nm))
        nframes, cap, npoints = int(d_n.numel()), int(cap_per_frame), int(npoints)
        nwin, nwin_kf, nobs = int(d_win_start.numel()) - 1, int(d_win_kf.numel()), int(d_obs_frame.numel())
        if cap < 1 or cap > Sim3Solver.MAX_N:
            raise ValueError("%s: cap_per_frame outside [1, %d]" % (name, Sim3Solver.MAX_N))
        if nwin < 0 or npoints < 0 or int(d_obs_start.numel()) != npoints + 1 or int(d_obs_idx.numel()) != nobs:
            raise ValueError("%s: d_win_start needs nwin + 1 entries, d_obs_start npoints + 1, d_obs_frame and d_obs_idx the same length" % name)
        if d_kf_point.numel() != nframes * cap or d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_pose.numel() * d_pose.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps, d_kf_point and d_pose must hold one row per frame of d_n" % name)
        if d_points.numel() * d_points.element_size() < npoints * MAP_POINT_DTYPE.itemsize:
            raise ValueError("%s: the table is shorter than npoints" % name)
        for nm, t_, need in (("d_point_bad", d_point_bad, npoints), ("d_kf_bad", d_kf_bad, nframes), ("d_kf_fixed_id0", d_kf_fixed_id0, nframes)):
            if t_ is not None and t_.numel() * t_.element_size() < need:
                raise ValueError("%s: %s is too short" % (name, nm))
        dev = d_n.device
        if d_pose_out is None:
            d_pose_out = d_pose.clone()
        elif d_pose_out.data_ptr() == d_pose.data_ptr() or d_pose_out.numel() * d_pose_out.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_pose_out must be another tensor of d_pose's size" % name)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(pose_out=d_pose_out, erase=z((max(nwin, 0), nobs), torch.uint8), chi2=z((max(nwin, 0), nobs), torch.float32),
                   level=z((max(nwin, 0), nobs), torch.uint8), is_local=z((max(nwin, 0), npoints), torch.uint8),
                   role=z((max(nwin, 0), nframes), torch.uint8), info=z((max(nwin, 0), LBA_INFO), torch.int32), nerased=z((max(nwin, 0),), torch.int32))
        q = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_local_bundle_adjustment_batch_device(
            ext._h, q(d_kps), q(d_n), nframes, cap, q(d_pose), q(d_kf_bad), q(d_kf_point), q(d_kf_fixed_id0), q(d_win_start), q(d_win_kf), nwin,
            nwin_kf, npoints, q(d_points), q(d_point_bad), q(d_obs_start), q(d_obs_frame), q(d_obs_idx), nobs, int(rounds), q(out["pose_out"]),
            q(out["erase"]), q(out["chi2"]), q(out["level"]), q(out["is_local"]), q(out["role"]), q(out["info"]), q(out["nerased"]), C.c_void_p(s)))
        return out

    @staticmethod
    def GlobalBundleAdjustment(key_frames, poses, points, obs_start, obs_frame, obs_idx, point_bad=None, kf_bad=None, kf_fixed_id0=None,
                               iterations=10, robust=False, in_place=False, ext=None):
        """Optimizer::GlobalBundleAdjustemnt (thirdparty/orb-slam2/src/Optimizer.cc:41-237, monocular) on the GPU.  key_frames:
        Frame-like objects IN RISING mnId ORDER (ext, N, mvKeysUndistorted: pt and octave are read); poses[f]: KF_POSE_DTYPE (Tcw and
        the camera are read); kf_bad[f] = isBad(), kf_fixed_id0[f] = (mnId == 0) (None = none).  points (MAP_POINT_DTYPE; pos is
        read), point_bad, and the observations as CSR of (obs_frame, obs_idx) as for RefreshMapPoints.  iterations: 10 from loop
        closing, 20 from initialisation; robust: RobustKernelHuber with (float)sqrt(5.99); in_place: the nLoopKF == 0 branch, the
        returned table then holds the done points' new positions.  Every input pgorb_global_bundle_adjustment refuses is a ValueError
        here, before the library is called; a map past a capacity (GBA_MAX_*) raises PgorbError.  Returns a dict: ret (the free
        active vertices), poses (every live key frame replaced), pos [npoints][3], kf_done, point_done, chi2 per observation, points
        (a copy of the table, written when in_place), status, edges, included_points, vertices, iterations, trials, envelope."""
        fn = "GlobalBundleAdjustment"
        nkf = len(key_frames)
        if ext is None:
            if not nkf:
                raise ValueError(fn + ": no key frame and no ext")
            ext = key_frames[0].ext
        if int(iterations) < 0:
            raise ValueError(fn + ": iterations is negative")
        if len(poses) != nkf:
            raise ValueError(fn + ": key_frames and poses differ in length")
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))       # a copy: moved in place
        n = len(pts)
        if not np.isfinite(pts["pos"]).all():
            raise ValueError(fn + ": a point is not finite")
        levels = ext.GetLevels()
        P = np.zeros(max(nkf, 1), KF_POSE_DTYPE)
        keep = []
        kps = (C.c_void_p * max(nkf, 1))()
        nk = np.zeros(max(nkf, 1), np.int32)
        octs = []
        for f, K in enumerate(key_frames):
            if int(K.N) < 0:
                raise ValueError("%s: key frame %d has a negative keypoint count" % (fn, f))
            kp = _arr(K.mvKeysUndistorted, KEYPOINT_DTYPE, K.N, "key frame %d keypoints" % f)
            kp_buf = kp if K.N else np.zeros(1, KEYPOINT_DTYPE)
            keep.append(kp_buf)
            kps[f], nk[f] = kp_buf.ctypes.data, K.N
            octs.append(kp["octave"])
            P[f] = np.asarray(poses[f], KF_POSE_DTYPE).reshape(())
            cam = [float(P[f][k]) for k in ("fx", "fy", "cx", "cy")]
            if not (np.isfinite(P[f]["Tcw"]).all() and np.isfinite(cam).all()):
                raise ValueError(fn + ": a pose or a camera is not finite")
            if cam[0] == 0.0 or cam[1] == 0.0:
                raise ValueError(fn + ": fx or fy is zero")
        kb, i0, pb = _mask(kf_bad, nkf, "kf_bad"), _mask(kf_fixed_id0, nkf, "kf_fixed_id0"), _mask(point_bad, n, "point_bad")
        st = _arr(obs_start, np.int32, n + 1, "obs_start")
        of = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
        oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
        if st[0] != 0 or np.any(np.diff(st) < 0) or len(of) < int(st[-1]) or len(oi) < int(st[-1]):
            raise ValueError(fn + ": obs_start must rise from 0 to at most len(obs_frame), len(obs_idx)")
        m = int(st[-1])
        if m and (of[:m].min() < 0 or of[:m].max() >= nkf or oi[:m].min() < 0 or np.any(oi[:m] >= nk[np.clip(of[:m], 0, max(nkf - 1, 0))])):
            raise ValueError(fn + ": an observation names a key frame or keypoint out of range")
        owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(st))
        if len(np.unique(owner * max(nkf, 1) + of[:m])) != m:
            raise ValueError(fn + ": a list names a key frame twice")
        for k in range(m):
            o = int(octs[of[k]][oi[k]])
            if o < 0 or o >= levels:
                raise ValueError("%s: an octave is outside the extractor's %d levels" % (fn, levels))
        if len(of) == 0:
            of, oi = np.zeros(1, np.int32), np.zeros(1, np.int32)
        po, pos = np.zeros(max(nkf, 1), KF_POSE_DTYPE), np.zeros((max(n, 1), 3), np.float32)
        kd, pd, chi = np.zeros(max(nkf, 1), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(max(m, 1), np.float32)
        info = np.zeros(GBA_INFO, np.int32)
        pts_buf = pts if n else np.zeros(1, MAP_POINT_DTYPE)
        ret = ext._check(ext._L.pgorb_global_bundle_adjustment(
            ext._h, nkf, kps, _p(nk), _p(P), _p(kb), _p(i0), n, _p(pts_buf), _p(pb), _p(st), _p(of), _p(oi), int(iterations), int(bool(robust)),
            int(bool(in_place)), _p(po), _p(pos), _p(kd), _p(pd), _p(chi), _p(info)))
        return dict(ret=ret, poses=po[:nkf].copy(), pos=pos[:n].copy(), kf_done=kd[:nkf].copy(), point_done=pd[:n].copy(), chi2=chi[:m].copy(),
                    points=pts, status=int(info[0]), edges=int(info[1]), included_points=int(info[2]), vertices=int(info[3]),
                    iterations=int(info[5]), trials=int(info[6]), envelope=int(info[7]))

    @staticmethod
    def GlobalBundleAdjustment_device(ext, d_kps, d_n, cap_per_frame, d_pose, npoints, d_points, d_obs_start, d_obs_frame, d_obs_idx,
                                      d_point_bad=None, d_kf_bad=None, d_kf_fixed_id0=None, iterations=10, robust=False, in_place=False,
                                      want_chi2=True, stream=None):
        """pgorb_global_bundle_adjustment_device over resident torch tensors: the frames of one batch in rising mnId order and the
        table.  The sizes and element types are checked here; the contents are not read.  Returns a dict of tensors: pose_out (bytes
        of KF_POSE_DTYPE per frame), pos_out [npoints][3], kf_done, point_done, chi2 [nobs] (None without want_chi2), info [GBA_INFO]
        (info[4] = the free active vertices).  With in_place d_points holds the done points' new positions and the chain into
        pMP->UpdateNormalAndDepth() is pgorb_refresh_map_points_batch_device on the same d_points with d_pose = pose_out."""
        import torch
        name = "Optimizer.GlobalBundleAdjustment_device"
        if int(iterations) < 0:
            raise ValueError(name + ": iterations is negative")
        for nm, t_ in (("d_n", d_n), ("d_obs_start", d_obs_start), ("d_obs_frame", d_obs_frame), ("d_obs_idx", d_obs_idx)):
            if t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the counts are taken from element counts)" % (name, nm))
        nframes, cap, npoints, nobs = int(d_n.numel()), int(cap_per_frame), int(npoints), int(d_obs_frame.numel())
        if cap < 1 or cap > Sim3Solver.MAX_N:
            raise ValueError("%s: cap_per_frame outside [1, %d]" % (name, Sim3Solver.MAX_N))
        if npoints < 0 or int(d_obs_start.numel()) != npoints + 1 or int(d_obs_idx.numel()) != nobs:
            raise ValueError("%s: d_obs_start needs npoints + 1 entries, d_obs_frame and d_obs_idx the same length" % name)
        if d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_pose.numel() * d_pose.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps and d_pose must hold one row per frame of d_n" % name)
        if d_points.numel() * d_points.element_size() < npoints * MAP_POINT_DTYPE.itemsize:
            raise ValueError("%s: the table is shorter than npoints" % name)
        for nm, t_, need in (("d_point_bad", d_point_bad, npoints), ("d_kf_bad", d_kf_bad, nframes), ("d_kf_fixed_id0", d_kf_fixed_id0, nframes)):
            if t_ is not None and t_.numel() * t_.element_size() < need:
                raise ValueError("%s: %s is too short" % (name, nm))
        dev = d_n.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(pose_out=torch.zeros_like(d_pose), pos_out=z((npoints, 3), torch.float32), kf_done=z((nframes,), torch.uint8),
                   point_done=z((npoints,), torch.uint8), chi2=z((nobs,), torch.float32) if want_chi2 else None, info=z((GBA_INFO,), torch.int32))
        q = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_global_bundle_adjustment_device(
            ext._h, q(d_kps), q(d_n), nframes, cap, q(d_pose), q(d_kf_bad), q(d_kf_fixed_id0), npoints, q(d_points), q(d_point_bad),
            C.c_void_p(d_obs_start.data_ptr()), q(d_obs_frame), q(d_obs_idx), nobs, int(iterations), int(bool(robust)), int(bool(in_place)),
            q(out["pose_out"]), q(out["pos_out"]), q(out["kf_done"]), q(out["point_done"]), q(out["chi2"]), C.c_void_p(out["info"].data_ptr()),
            C.c_void_p(s)))
        return out

    @staticmethod
    def check_essential_graph(name, kf_id, poses, loop_kf, cur_kf, parent, loop_conn, loop_edge_start, loop_edge, covis_start, covis, covis_weight,
                              points, point_ref_kf, kf_bad, point_bad, has_corrected, corrected, has_non_corrected, non_corrected, iterations):
        """pgorb_optimize_essential_graph's checks, without a device; returns the arrays the library reads."""
        ids = np.ascontiguousarray(kf_id, np.uint64).reshape(-1)
        nkf = len(ids)
        if nkf and np.any(np.diff(ids.astype(object)) <= 0):
            raise ValueError("%s: kf_id is not strictly rising" % name)
        if int(iterations) < 0:
            raise ValueError("%s: iterations is negative" % name)
        P = np.ascontiguousarray(poses, KF_POSE_DTYPE).reshape(-1)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        if len(P) != nkf or len(par) != nkf:
            raise ValueError("%s: kf_id, poses and parent differ in length" % name)
        if not np.isfinite(P["Tcw"]).all():
            raise ValueError("%s: a pose is not finite" % name)
        if nkf and not (0 <= int(loop_kf) < nkf and 0 <= int(cur_kf) < nkf):
            raise ValueError("%s: loop_kf or cur_kf is out of range" % name)
        if nkf and (int(par.min()) < -1 or int(par.max()) >= nkf or np.any(par == np.arange(nkf))):
            raise ValueError("%s: a parent is out of range" % name)
        maps = []
        for nm, has, rec in (("corrected", has_corrected, corrected), ("non_corrected", has_non_corrected, non_corrected)):
            if has is None:
                maps += [None, None]
                continue
            h = _arr(has, np.uint8, nkf, "has_" + nm)
            if rec is None:
                raise ValueError("%s: has_%s without %s" % (name, nm, nm))
            r = np.ascontiguousarray(rec, SIM3D_DTYPE).reshape(-1)
            if len(r) != nkf:
                raise ValueError("%s: %s needs one record per key frame" % (name, nm))
            u = h != 0
            if u.any() and not (np.isfinite(r["r"][u]).all() and np.isfinite(r["t"][u]).all() and np.isfinite(r["s"][u]).all() and (r["s"][u] > 0).all()):
                raise ValueError("%s: a Sim3 of %s is not finite or its scale is not positive" % (name, nm))
            maps += [h, r]
        lc = np.ascontiguousarray(loop_conn, np.int32).reshape(-1, 3)
        if len(lc) and (not nkf or int(lc[:, :2].min()) < 0 or int(lc[:, :2].max()) >= nkf or np.any(lc[:, 0] == lc[:, 1])):
            raise ValueError("%s: a loop connection is out of range or joins a key frame to itself" % name)
        rows = []
        for nm, st, vals in (("loop_edge", loop_edge_start, [loop_edge]), ("covis", covis_start, [covis, covis_weight])):
            s = _arr(st, np.int32, nkf + 1, nm + "_start")
            if s[0] != 0 or np.any(np.diff(s) < 0):
                raise ValueError("%s: %s_start must rise from 0" % (name, nm))
            m = int(s[-1])
            vs = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in vals]
            if any(len(v) < m for v in vs):
                raise ValueError("%s: %s is shorter than its start array says" % (name, nm))
            own = np.repeat(np.arange(nkf, dtype=np.int64), np.diff(s))
            if m and (int(vs[0][:m].min()) < 0 or int(vs[0][:m].max()) >= nkf or np.any(vs[0][:m] == own)):
                raise ValueError("%s: a %s entry is out of range or names its own key frame" % (name, nm))
            rows += [s] + [v[:m] if m else np.zeros(1, np.int32) for v in vs]
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))      # a copy: moved in place
        ref = np.ascontiguousarray(point_ref_kf, np.int32).reshape(-1)
        if len(ref) != len(pts):
            raise ValueError("%s: point_ref_kf needs one entry per point" % name)
        if len(pts) and (int(ref.min()) < -1 or int(ref.max()) >= nkf):
            raise ValueError("%s: point_ref_kf is out of range" % name)
        if not np.isfinite(pts["pos"]).all():
            raise ValueError("%s: a point is not finite" % name)
        return dict(nkf=nkf, ids=ids, P=P, par=par, maps=maps, lc=lc, rows=rows, pts=pts, ref=ref, kb=_mask(kf_bad, nkf, "kf_bad"),
                    pb=_mask(point_bad, len(pts), "point_bad"))

    @staticmethod
    def OptimizeEssentialGraph(ext, kf_id, poses, loop_kf, cur_kf, parent, loop_conn, loop_edge_start, loop_edge, covis_start, covis, covis_weight,
                               points, point_ref_kf, kf_bad=None, point_bad=None, has_corrected=None, corrected=None, has_non_corrected=None,
                               non_corrected=None, bFixScale=False, min_feat=100, iterations=20):
        """Optimizer::OptimizeEssentialGraph (thirdparty/orb-slam2/src/Optimizer.cc:781-1044) on the GPU: the call of
        LoopClosing::CorrectLoop after SearchAndFuse.  Key frames by index in strictly rising kf_id (mnId) order with their
        KF_POSE_DTYPE poses; loop_kf, cur_kf by index; corrected / non_corrected = CorrectedSim3 / NonCorrectedSim3 as SIM3D_DTYPE
        records with their has_ flags (None = an empty map); loop_conn [m][3] = (i, j, weight) in LoopConnections' iteration order;
        parent[i] or -1; GetLoopEdges() and the covisibles with weights as CSR per key frame; points (MAP_POINT_DTYPE; pos is read)
        with point_ref_kf[p] = the key frame Optimizer.cc:1020-1029 selects, or -1.  The filters, the edge order and the
        measurements are derived on the device (include/pgorb.h).  Every input pgorb_optimize_essential_graph refuses is a
        ValueError here, before the library is called; a graph past a capacity (EG_MAX_*) raises PgorbError.  Returns a dict: ret
        (the optimised vertices), poses, sim3 (SIM3D_DTYPE), points (a copy with pos corrected), edges (EG_EDGE_DTYPE: the
        derived edges with their final chi2), status, vertices, free, kinds (edges per kind), iterations, trials, envelope."""
        a = Optimizer.check_essential_graph("OptimizeEssentialGraph", kf_id, poses, loop_kf, cur_kf, parent, loop_conn, loop_edge_start, loop_edge,
                                            covis_start, covis, covis_weight, points, point_ref_kf, kf_bad, point_bad, has_corrected, corrected,
                                            has_non_corrected, non_corrected, iterations)
        nkf, n = a["nkf"], len(a["pts"])
        hc, cor, hn, non = a["maps"]
        ls, le, cs, cv, cw = a["rows"]
        ncand = len(a["lc"]) + nkf + int(ls[-1]) + int(cs[-1])
        k1 = max(nkf, 1)
        so, po, eo = np.zeros(k1, SIM3D_DTYPE), np.zeros(k1, KF_POSE_DTYPE), np.zeros(max(ncand, 1), EG_EDGE_DTYPE)
        info = np.zeros(EG_INFO, np.int32)
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
        q = lambda x: None if x is None else _p(x)
        ret = ext._check(ext._L.pgorb_optimize_essential_graph(
            ext._h, nkf, _p(pad(a["ids"], np.uint64)), _p(pad(a["P"], KF_POSE_DTYPE)), _p(a["kb"]), int(loop_kf), int(cur_kf), int(bool(bFixScale)),
            q(hc), q(cor), q(hn), q(non), len(a["lc"]), _p(pad(a["lc"].reshape(-1), np.int32)), _p(pad(a["par"], np.int32)), _p(ls), _p(le), _p(cs),
            _p(cv), _p(cw), int(min_feat), int(iterations), n, _p(pad(a["pts"], MAP_POINT_DTYPE)), _p(a["pb"]), _p(pad(a["ref"], np.int32)), _p(so),
            _p(po), _p(eo), _p(info)))
        ne = int(info[3:7].sum())
        return dict(ret=ret, poses=po[:nkf].copy(), sim3=so[:nkf].copy(), points=a["pts"], edges=eo[:ne].copy(), status=int(info[0]),
                    vertices=int(info[1]), free=int(info[2]), kinds=[int(x) for x in info[3:7]], iterations=int(info[7]), trials=int(info[8]),
                    envelope=int(info[9]))

    @staticmethod
    def OptimizeEssentialGraph_device(ext, d_kf_id, d_pose, loop_kf, cur_kf, d_parent, d_loop_conn, d_loop_edge_start, d_loop_edge, d_covis_start,
                                      d_covis, d_covis_weight, npoints, d_points, d_point_ref_kf, d_kf_bad=None, d_point_bad=None,
                                      d_has_corrected=None, d_corrected=None, d_has_non_corrected=None, d_non_corrected=None, bFixScale=False,
                                      min_feat=100, iterations=20, want_edges=True, stream=None):
        """pgorb_optimize_essential_graph_device over resident torch tensors, asynchronous on `stream`: d_kf_id int64 (the bits of the
        uint64 mnId), d_pose / d_corrected / d_non_corrected / d_points the bytes of their dtypes, the lists int32, the flags uint8.
        The sizes and element types are checked here (an empty key-frame list is refused here, although the library answers it with
        EG_NOTHING); the contents are not read: a list entry out of range is no candidate.  d_points
        is corrected IN PLACE.  Returns a dict of freshly allocated tensors: pose_out, sim3_out (bytes of their dtypes per key
        frame), edge_out (bytes of EG_EDGE_DTYPE per candidate; info[3:7] count the valid records; None without want_edges) and
        info [EG_INFO].  The chain into pMP->UpdateNormalAndDepth() is pgorb_refresh_map_points_batch_device on the same d_points
        with d_pose = pose_out."""
        import torch
        name = "Optimizer.OptimizeEssentialGraph_device"
        if int(iterations) < 0:
            raise ValueError(name + ": iterations is negative")
        for nm, t_ in (("d_parent", d_parent), ("d_loop_conn", d_loop_conn), ("d_loop_edge_start", d_loop_edge_start), ("d_loop_edge", d_loop_edge),
                       ("d_covis_start", d_covis_start), ("d_covis", d_covis), ("d_covis_weight", d_covis_weight), ("d_point_ref_kf", d_point_ref_kf)):
            if t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the counts are taken from element counts)" % (name, nm))
        if d_kf_id.dtype != torch.int64:
            raise ValueError(name + ": d_kf_id must be an int64 tensor")
        nkf, npoints = int(d_kf_id.numel()), int(npoints)
        nlc, nle, ncv = int(d_loop_conn.numel()) // 3, int(d_loop_edge.numel()), int(d_covis.numel())
        if not nkf or not (0 <= int(loop_kf) < nkf and 0 <= int(cur_kf) < nkf):
            raise ValueError(name + ": no key frame, or loop_kf or cur_kf is out of range")
        if int(d_parent.numel()) != nkf or int(d_loop_edge_start.numel()) != nkf + 1 or int(d_covis_start.numel()) != nkf + 1 or \
                int(d_covis_weight.numel()) != ncv or int(d_loop_conn.numel()) != 3 * nlc or \
                d_pose.numel() * d_pose.element_size() != nkf * KF_POSE_DTYPE.itemsize:
            raise ValueError(name + ": d_pose and d_parent need one entry per key frame, the start arrays nkf + 1, d_covis_weight one per covisible")
        if npoints < 0 or d_points.numel() * d_points.element_size() < npoints * MAP_POINT_DTYPE.itemsize or int(d_point_ref_kf.numel()) < npoints:
            raise ValueError(name + ": the table or d_point_ref_kf is shorter than npoints")
        for nm, has, rec in (("corrected", d_has_corrected, d_corrected), ("non_corrected", d_has_non_corrected, d_non_corrected)):
            if has is not None and (rec is None or has.numel() * has.element_size() != nkf or rec.numel() * rec.element_size() != nkf * SIM3D_DTYPE.itemsize):
                raise ValueError("%s: d_has_%s needs one byte and d_%s one record per key frame" % (name, nm, nm))
        for nm, t_, need in (("d_kf_bad", d_kf_bad, nkf), ("d_point_bad", d_point_bad, npoints)):
            if t_ is not None and t_.numel() * t_.element_size() < need:
                raise ValueError("%s: %s is too short" % (name, nm))
        dev = d_kf_id.device
        ncand = nlc + nkf + nle + ncv
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(pose_out=z((nkf, KF_POSE_DTYPE.itemsize), torch.uint8), sim3_out=z((nkf, SIM3D_DTYPE.itemsize), torch.uint8),
                   edge_out=z((ncand, EG_EDGE_DTYPE.itemsize), torch.uint8) if want_edges else None, info=z((EG_INFO,), torch.int32))
        q = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_optimize_essential_graph_device(
            ext._h, nkf, q(d_kf_id), q(d_pose), q(d_kf_bad), int(loop_kf), int(cur_kf), int(bool(bFixScale)), q(d_has_corrected),
            q(d_corrected) if d_has_corrected is not None else None, q(d_has_non_corrected), q(d_non_corrected) if d_has_non_corrected is not None else None,
            nlc, q(d_loop_conn), q(d_parent), q(d_loop_edge_start), q(d_loop_edge), nle, q(d_covis_start), q(d_covis), q(d_covis_weight), ncv,
            int(min_feat), int(iterations), npoints, q(d_points), q(d_point_bad), q(d_point_ref_kf), q(out["sim3_out"]), q(out["pose_out"]),
            q(out["edge_out"]), q(out["info"]), C.c_void_p(s)))
        return out


class Sim3Solver:
    """Sim3Solver (thirdparty/orb-slam2/src/Sim3Solver.cc) on the GPU, with the reference's surface: the constructor,
    SetRansacParameters, iterate(n), find and the three getters.  mnIterations and mnBestInliers live here and go to the library
    as first_iteration / best_inliers_in, so iterate(5) can be called again on the same solver as LoopClosing::ComputeSim3 does.

    KF1, KF2: Frame-like objects (ext, N, mvKeysUndistorted: the octave is read); pose1, pose2: KF_POSE_DTYPE records (Tcw and each
    key frame's own camera are read); kf_point1 / kf_point2: the table index of every slot's point or -1 (the caller owns
    GetIndexInKeyFrame); matches12[i1]: the KF2 keypoint SearchByBoW matched, or -1; table: a MapPointTable (pos and bad are read).
    draws: [>= maxIterations][3] raw rand() values in [0, 2^31); None draws them from numpy's RandomState(seed).  Every input
    the library's checked call refuses is a ValueError here, before the library is called."""
    MAX_N = 16000

    def __init__(self, KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, table, bFixScale=False, draws=None, seed=0):
        if draws is not None:
            self.check_params("Sim3Solver", 0.99, 6, 1, draws=draws)
        self._a = self.check("Sim3Solver", KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, table)
        self.ext, self.table = KF1.ext, table
        self.mbFixScale = bool(bFixScale)
        self._draws_in, self._seed = draws, seed
        self.mnIterations, self.mnBestInliers = 0, 0
        self.best = np.zeros((), SIM3_ESTIMATE_DTYPE)
        self.found_sim3 = np.zeros((), SIM3_DTYPE)
        self.matches12_out = self.already1 = self.already2 = None
        self.info = np.zeros(S3_INFO, np.int32)
        self.SetRansacParameters()

    @staticmethod
    def check(name, KF1, KF2, pose1, pose2, kf_point1, kf_point2, matches12, table):
        """The single call's checks of the key frames and the table, without a device; returns the arrays the library reads."""
        n1, n2 = int(KF1.N), int(KF2.N)
        if n1 < 0 or n2 < 0:
            raise ValueError("%s: a negative keypoint count" % name)
        k1 = _arr(KF1.mvKeysUndistorted, KEYPOINT_DTYPE, n1, name + " KF1 keypoints")
        k2 = _arr(KF2.mvKeysUndistorted, KEYPOINT_DTYPE, n2, name + " KF2 keypoints")
        s1, s2 = _arr(kf_point1, np.int32, n1, "kf_point1"), _arr(kf_point2, np.int32, n2, "kf_point2")
        m = _arr(matches12, np.int32, n1, "matches12")
        table.check_indices(s1, "kf_point1", name)
        table.check_indices(s2, "kf_point2", name)
        if n1 and (int(m.min()) < -1 or int(m.max()) >= n2):
            raise ValueError("%s: matches12 is outside [-1, n2)" % name)
        P1, P2 = (np.ascontiguousarray(P, KF_POSE_DTYPE).reshape(()) for P in (pose1, pose2))
        for P in (P1, P2):
            if not (np.isfinite(P["Tcw"]).all() and np.isfinite([float(P[k]) for k in ("fx", "fy", "cx", "cy")]).all()):
                raise ValueError("%s: a pose or a camera is not finite" % name)
        i1 = np.nonzero(m >= 0)[0]
        i1 = i1[(s1[i1] >= 0) & (s2[m[i1]] >= 0)]
        if len(i1):
            if not (np.isfinite(table.points["pos"][s1[i1]]).all() and np.isfinite(table.points["pos"][s2[m[i1]]]).all()):
                raise ValueError("%s: a referenced point is not finite" % name)
            levels = KF1.ext.GetLevels()
            o = np.concatenate([k1["octave"][i1], k2["octave"][m[i1]]])
            if int(o.min()) < 0 or int(o.max()) >= levels:
                raise ValueError("%s: an octave is outside the extractor's %d levels" % (name, levels))
        if max(n1, n2) > Sim3Solver.MAX_N:
            raise ValueError("%s: more than %d keypoints in a key frame" % (name, Sim3Solver.MAX_N))
        return dict(n1=n1, n2=n2, k1=k1, k2=k2, s1=s1, s2=s2, m=m, P1=P1, P2=P2)

    @staticmethod
    def check_params(name, probability, minInliers, maxIterations, first_iteration=0, niterations=1, draws=None):
        """The single call's checks of the parameter block and the draws."""
        if int(minInliers) < 3:
            raise ValueError("%s: minInliers is below 3" % name)
        if not 0.0 < float(np.float32(probability)) < 1.0:
            raise ValueError("%s: probability is outside (0, 1)" % name)
        if int(maxIterations) < 1:
            raise ValueError("%s: maxIterations is below 1" % name)
        if int(first_iteration) < 0:
            raise ValueError("%s: first_iteration is negative" % name)
        if int(niterations) < 1:
            raise ValueError("%s: niterations is below 1" % name)
        if int(maxIterations) > SIM3_MAX_ITERATIONS:
            raise ValueError("%s: maxIterations above %d" % (name, SIM3_MAX_ITERATIONS))
        if draws is not None:
            d = np.asarray(draws)
            if d.ndim < 2 or d.shape[-1] != 3 or d.shape[-2] < int(maxIterations):
                raise ValueError("%s: draws must be [maxIterations][3]" % name)
            if d.size and (int(d.min()) < 0 or int(d.max()) >= 2 ** 31):
                raise ValueError("%s: a draw is not in [0, 2^31)" % name)

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """Sim3Solver.cc:114-138; resets mnIterations as the reference does (mnBestInliers stays)."""
        self.check_params("SetRansacParameters", probability, minInliers, maxIterations, draws=self._draws_in)
        self.mRansacProb, self.mRansacMinInliers, self.mRansacMaxIts = float(probability), int(minInliers), int(maxIterations)
        if self._draws_in is None:
            self.draws = np.random.RandomState(self._seed).randint(0, 2 ** 31, (self.mRansacMaxIts, 3)).astype(np.uint32)
        else:
            self.draws = np.ascontiguousarray(np.asarray(self._draws_in)[:self.mRansacMaxIts], np.uint32)
        self.mnIterations = 0

    def iterate(self, nIterations):
        """Sim3Solver::iterate (:140-207).  Returns (T12, bNoMore, vbInliers, nInliers): T12 the 4 x 4 float [s*R | t] of the
        returned hypothesis or None."""
        self.check_params("iterate", self.mRansacProb, self.mRansacMinInliers, self.mRansacMaxIts, self.mnIterations, nIterations)
        a, ext, t = self._a, self.ext, self.table
        prm = np.zeros(1, SIM3_PARAMS_DTYPE)
        prm["probability"], prm["min_inliers"], prm["max_iterations"] = self.mRansacProb, self.mRansacMinInliers, self.mRansacMaxIts
        prm["fix_scale"], prm["first_iteration"], prm["niterations"] = int(self.mbFixScale), self.mnIterations, min(int(nIterations), 2 ** 30)
        prm["best_inliers_in"] = self.mnBestInliers
        n1, n2 = a["n1"], a["n2"]
        found, best, sim3 = np.zeros(1, SIM3_ESTIMATE_DTYPE), np.zeros(1, SIM3_ESTIMATE_DTYPE), np.zeros(1, SIM3_DTYPE)
        fl, mo, a1, a2 = np.zeros(max(n1, 1), np.uint8), np.full(max(n1, 1), -1, np.int32), np.zeros(max(n1, 1), np.uint8), np.zeros(max(n2, 1), np.uint8)
        info = np.zeros(S3_INFO, np.int32)
        pad = lambda x, n, dt: x if n else np.zeros(1, dt)
        ret = ext._check(ext._L.pgorb_sim3_solver(
            ext._h, _p(pad(a["k1"], n1, KEYPOINT_DTYPE)), n1, _p(a["P1"]), _p(pad(a["s1"], n1, np.int32)), _p(pad(a["k2"], n2, KEYPOINT_DTYPE)), n2,
            _p(a["P2"]), _p(pad(a["s2"], n2, np.int32)), _p(pad(a["m"], n1, np.int32)), t.n, _p(t.points), _p(t.bad), _p(prm), _p(self.draws),
            _p(found), _p(sim3), _p(best), _p(fl), _p(mo), _p(a1), _p(a2), _p(info)))
        self.info = info
        self.mnIterations, self.mnBestInliers = int(info[3]), int(info[5])
        if info[6] >= 0:
            self.best = best[0].copy()
        self.found, self.found_sim3 = found[0].copy(), sim3[0].copy()
        self.matches12_out, self.already1, self.already2 = mo[:n1].copy(), a1[:n1].copy(), a2[:n2].copy()
        no_more = bool(info[0] & (S3_FEW | S3_NO_MORE))
        T12 = None
        if info[0] & S3_FOUND:
            T12 = np.eye(4, dtype=np.float32)
            T12[:3, :3], T12[:3, 3] = sim3[0]["sR12"].reshape(3, 3), sim3[0]["t12"]
        return T12, no_more, fl[:n1].astype(bool), int(ret)

    def find(self):
        """Sim3Solver::find (:209-213): iterate(mRansacMaxIts).  Returns (T12, vbInliers12, nInliers)."""
        T12, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T12, inl, n

    def GetEstimatedRotation(self):
        return self.best["R12"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self.best["t12"].copy()

    def GetEstimatedScale(self):
        return float(self.best["s12"])

    @staticmethod
    def iterate_batch_device(ext, d_kps, d_n, cap_per_frame, d_pair_kf1, d_pair_kf2, d_pose, d_kf_point, d_matches12, npoints, d_points,
                             d_point_bad, d_draws, probability=0.99, minInliers=20, maxIterations=300, nIterations=300, bFixScale=False,
                             first_iteration=0, best_inliers_in=0, d_first_iteration=None, d_best_inliers_in=None, stream=None):
        """pgorb_sim3_solver_batch_device over resident torch tensors: pair p aligns key frames d_pair_kf1[p] and d_pair_kf2[p];
        d_draws is [npairs][maxIterations][3] uint32 (or int32 bits).  The parameters and the sizes are checked here as the single
        call checks them, and the tensors' element types and sizes against npairs, cap and the number of frames (the pair count is
        d_pair_kf1's element count, so the index tensors must be int32); the arrays' contents are not read: the batched form counts
        a bad index as no correspondence and trusts the pair lists.  Returns a
        dict of freshly allocated tensors: found, found_sim3, best (bytes of their dtypes per pair), inlier, matches12_out,
        already1, already2 [npairs][cap], info [npairs][S3_INFO], ninliers [npairs]."""
        import torch
        name = "Sim3Solver.iterate_batch_device"
        Sim3Solver.check_params(name, probability, minInliers, maxIterations, first_iteration, nIterations)
        for nm, t_ in (("d_pair_kf1", d_pair_kf1), ("d_pair_kf2", d_pair_kf2), ("d_matches12", d_matches12), ("d_n", d_n), ("d_kf_point", d_kf_point),
                       ("d_first_iteration", d_first_iteration), ("d_best_inliers_in", d_best_inliers_in)):
            if t_ is not None and t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the pair count and the row lengths are taken from element counts)" % (name, nm))
        if d_draws.element_size() != 4:
            raise ValueError("%s: d_draws must have 4-byte elements" % name)
        npairs, cap = int(d_pair_kf1.numel()), int(cap_per_frame)
        if cap < 1 or cap > Sim3Solver.MAX_N:
            raise ValueError("%s: cap_per_frame outside [1, %d]" % (name, Sim3Solver.MAX_N))
        if int(d_pair_kf2.numel()) != npairs or int(npoints) < 0:
            raise ValueError("%s: the pair lists differ in length or npoints is negative" % name)
        if d_matches12.numel() != npairs * cap or d_draws.numel() != npairs * int(maxIterations) * 3:
            raise ValueError("%s: d_matches12 must be [npairs][cap] and d_draws [npairs][maxIterations][3]" % name)
        nframes = int(d_n.numel())
        if d_kf_point.numel() != nframes * cap or d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_pose.numel() * d_pose.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps, d_kf_point and d_pose must hold one row per frame of d_n" % name)
        if d_points.numel() * d_points.element_size() < int(npoints) * MAP_POINT_DTYPE.itemsize or \
                (d_point_bad is not None and d_point_bad.numel() * d_point_bad.element_size() < int(npoints)):
            raise ValueError("%s: the table is shorter than npoints" % name)
        dev = d_matches12.device
        prm = np.zeros(1, SIM3_PARAMS_DTYPE)
        prm["probability"], prm["min_inliers"], prm["max_iterations"] = probability, minInliers, maxIterations
        prm["fix_scale"], prm["first_iteration"], prm["niterations"], prm["best_inliers_in"] = int(bool(bFixScale)), first_iteration, nIterations, best_inliers_in
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(found=e((npairs, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8), found_sim3=e((npairs, SIM3_DTYPE.itemsize), torch.uint8),
                   best=e((npairs, SIM3_ESTIMATE_DTYPE.itemsize), torch.uint8), inlier=e((npairs, cap), torch.uint8),
                   matches12_out=e((npairs, cap), torch.int32), already1=e((npairs, cap), torch.uint8), already2=e((npairs, cap), torch.uint8),
                   info=e((npairs, S3_INFO), torch.int32), ninliers=e((npairs,), torch.int32))
        q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_sim3_solver_batch_device(
            ext._h, q(d_kps), q(d_n), cap, q(d_pair_kf1), q(d_pair_kf2), npairs, q(d_pose), q(d_kf_point), q(d_matches12), int(npoints), q(d_points),
            q(d_point_bad), _p(prm), q(d_first_iteration), q(d_best_inliers_in), q(d_draws), q(out["found"]), q(out["found_sim3"]), q(out["best"]),
            q(out["inlier"]), q(out["matches12_out"]), q(out["already1"]), q(out["already2"]), q(out["info"]), q(out["ninliers"]), C.c_void_p(s)))
        return out


# pgorb_pnp_solver: the parameter block, a traced hypothesis, the status bits and the limits (include/pgorb.h)
PNP_PARAMS_DTYPE = np.dtype([("probability", "<f4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("min_set", "<i4"), ("epsilon", "<f4"),
                             ("th2", "<f4"), ("first_iteration", "<i4"), ("niterations", "<i4"), ("best_inliers_in", "<i4")])
PNP_HYPOTHESIS_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("inliers", "<i4"), ("flags", "<i4")])
PNP_FEW, PNP_FOUND, PNP_NO_MORE, PNP_REFINED, PNP_INFO, PNP_MAX_WINDOW = 1, 2, 4, 8, 8, 1024


class PnPsolver:
    """PnPsolver (thirdparty/orb-slam2/src/PnPsolver.cc) on the GPU, with the reference's surface: the constructor,
    SetRansacParameters, iterate(n) and find.  mnIterations, mnBestInliers, mvbBestInliers (by keypoint) and mBestTcw live here and
    go to the library with every call, so iterate(5) can be called again on the same solver as Tracking::Relocalization does.

    F: a Frame-like object (ext, N, mvKeysUndistorted: pt and octave are read); camera: a KF_POSE_DTYPE record (fx, fy, cx, cy are
    read); kp_point: the table index of vpMapPointMatches[i] or -1; table: a MapPointTable (pos and bad are read).  draws:
    [>= max(maxIterations, nIterations)][4] raw rand() values in [0, 2^31); None draws them from numpy's RandomState(seed).
    Every input the library's checked call refuses is a ValueError here, before the library is called."""
    MAX_N = 16000

    def __init__(self, F, camera, kp_point, table, draws=None, seed=0):
        self._a = self.check("PnPsolver", F, camera, kp_point, table)
        self.ext, self.table = F.ext, table
        self._draws_in, self._seed = draws, seed
        self.mnIterations, self.mnBestInliers = 0, 0
        self.mvbBestInliers = np.zeros(max(self._a["n"], 1), np.uint8)
        self.mBestTcw = np.zeros(1, KF_POSE_DTYPE)
        self.pose = np.zeros((), KF_POSE_DTYPE)
        self.kp_point_out = None
        self.info = np.zeros(PNP_INFO, np.int32)
        self.SetRansacParameters()

    @staticmethod
    def check(name, F, camera, kp_point, table):
        """The single call's checks of the frame and the table, without a device; returns the arrays the library reads."""
        n = int(F.N)
        if n < 0:
            raise ValueError("%s: a negative keypoint count" % name)
        k = _arr(F.mvKeysUndistorted, KEYPOINT_DTYPE, n, name + " keypoints")
        s = _arr(kp_point, np.int32, n, "kp_point")
        table.check_indices(s, "kp_point", name)
        P = np.ascontiguousarray(camera, KF_POSE_DTYPE).reshape(())
        if not np.isfinite([float(P[q]) for q in ("fx", "fy", "cx", "cy")]).all():
            raise ValueError("%s: the camera is not finite" % name)
        i = np.nonzero(s >= 0)[0]
        if table.bad is not None and len(i):
            i = i[np.asarray(table.bad)[s[i]] == 0]
        if len(i):
            if not (np.isfinite(table.points["pos"][s[i]]).all() and np.isfinite(k["x"][i]).all() and np.isfinite(k["y"][i]).all()):
                raise ValueError("%s: a referenced point or keypoint is not finite" % name)
            levels = F.ext.GetLevels()
            if int(k["octave"][i].min()) < 0 or int(k["octave"][i].max()) >= levels:
                raise ValueError("%s: an octave is outside the extractor's %d levels" % (name, levels))
        if n > PnPsolver.MAX_N:
            raise ValueError("%s: more than %d keypoints in the frame" % (name, PnPsolver.MAX_N))
        return dict(n=n, k=k, s=s, P=P)

    @staticmethod
    def check_params(name, probability, minInliers, maxIterations, minSet, epsilon, th2, first_iteration=0, niterations=1, draws=None):
        """The single call's checks of the parameter block and the draws."""
        if int(minSet) != 4:
            raise ValueError("%s: minSet must be 4" % name)
        if int(minInliers) < 1:
            raise ValueError("%s: minInliers is below 1" % name)
        if not 0.0 < float(np.float32(probability)) < 1.0:
            raise ValueError("%s: probability is outside (0, 1)" % name)
        if not 0.0 < float(np.float32(epsilon)) <= 1.0:
            raise ValueError("%s: epsilon is outside (0, 1]" % name)
        if not float(np.float32(th2)) > 0.0:
            raise ValueError("%s: th2 is not positive" % name)
        if int(maxIterations) < 1 or int(niterations) < 1 or int(first_iteration) < 0:
            raise ValueError("%s: maxIterations or nIterations below 1, or a negative first iteration" % name)
        W = max(int(maxIterations), int(niterations))
        if W > PNP_MAX_WINDOW:
            raise ValueError("%s: a window above %d" % (name, PNP_MAX_WINDOW))
        if draws is not None:
            d = np.asarray(draws)
            if d.ndim < 2 or d.shape[-1] != 4 or d.shape[-2] < W:
                raise ValueError("%s: draws must be [max(maxIterations, nIterations)][4]" % name)
            if d.size and (int(d.min()) < 0 or int(d.max()) >= 2 ** 31):
                raise ValueError("%s: a draw is not in [0, 2^31)" % name)
        return W

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        """PnPsolver.cc:121-157 (the header's defaults).  The adjusted minimum and the cap come from pgorb_pnp_ransac."""
        self.check_params("SetRansacParameters", probability, minInliers, maxIterations, minSet, epsilon, th2)
        self._prm = (float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon), float(th2))
        mi, cap = C.c_int32(0), C.c_int32(0)
        N = int(((self._a["s"] >= 0) & ((np.asarray(self.table.bad)[np.maximum(self._a["s"], 0)] == 0) if self.table.bad is not None else True)).sum())
        self.ext._L.pgorb_pnp_ransac(C.c_float(probability), int(minInliers), int(maxIterations), int(minSet), C.c_float(epsilon), N,
                                     C.byref(mi), C.byref(cap))
        self.N, self.mRansacMinInliers, self.mRansacMaxIts = N, int(mi.value), int(cap.value)

    def iterate(self, nIterations):
        """PnPsolver::iterate (:165-258).  Returns (Tcw, bNoMore, vbInliers, nInliers): Tcw the 4 x 4 float pose or None."""
        pr, mi, mx, ms, eps, th2 = self._prm
        W = self.check_params("iterate", pr, mi, mx, ms, eps, th2, self.mnIterations, nIterations, self._draws_in)
        if self._draws_in is None:
            draws = np.random.RandomState(self._seed + self.mnIterations).randint(0, 2 ** 31, (W, 4)).astype(np.uint32)
        else:
            draws = np.ascontiguousarray(np.asarray(self._draws_in)[:W], np.uint32)
        a, ext, t = self._a, self.ext, self.table
        prm = np.zeros(1, PNP_PARAMS_DTYPE)
        prm["probability"], prm["min_inliers"], prm["max_iterations"], prm["min_set"], prm["epsilon"], prm["th2"] = pr, mi, mx, ms, eps, th2
        prm["first_iteration"], prm["niterations"], prm["best_inliers_in"] = self.mnIterations, int(nIterations), self.mnBestInliers
        n = a["n"]
        pose, bpose = np.zeros(1, KF_POSE_DTYPE), np.zeros(1, KF_POSE_DTYPE)
        fl, kpo, bi = np.zeros(max(n, 1), np.uint8), np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.uint8)
        info = np.zeros(PNP_INFO, np.int32)
        pad = lambda x, dt: x if n else np.zeros(1, dt)
        ret = ext._check(ext._L.pgorb_pnp_solver(
            ext._h, _p(pad(a["k"], KEYPOINT_DTYPE)), n, _p(a["P"]), _p(pad(a["s"], np.int32)), t.n, _p(t.points), _p(t.bad), _p(prm), _p(draws),
            _p(self.mvbBestInliers), _p(self.mBestTcw), _p(pose), _p(fl), _p(kpo), _p(bi), _p(bpose), None, _p(info)))
        self.info = info
        self.mnIterations, self.mnBestInliers = int(info[4]), int(info[6])
        self.mvbBestInliers, self.mBestTcw = bi, bpose
        self.pose, self.kp_point_out = pose[0].copy(), kpo[:n].copy()
        Tcw = None
        if info[0] & PNP_FOUND:
            Tcw = np.eye(4, dtype=np.float32)
            Tcw[:3, :] = pose[0]["Tcw"].reshape(3, 4)
        return Tcw, bool(info[0] & PNP_NO_MORE), fl[:n].astype(bool), int(ret)

    def find(self):
        """PnPsolver::find (:159-163): iterate(mRansacMaxIts).  Returns (Tcw, vbInliers, nInliers)."""
        Tcw, _, inl, n = self.iterate(self.mRansacMaxIts)
        return Tcw, inl, n

    @staticmethod
    def iterate_batch_device(ext, d_kps, d_n, cap_per_frame, d_pair_frame, npairs, d_camera, d_kp_point, npoints, d_points, d_point_bad, d_draws,
                             probability=0.99, minInliers=10, maxIterations=300, minSet=4, epsilon=0.5, th2=5.991, nIterations=5,
                             first_iteration=0, best_inliers_in=0, d_first_iteration=None, d_best_inliers_in=None, d_best_inlier=None,
                             d_best_pose=None, trace=False, stream=None):
        """pgorb_pnp_solver_batch_device over resident torch tensors (the defaults are Tracking::Relocalization's): pair p solves frame
        d_pair_frame[p] (None: frame p); d_kp_point is [npairs][cap]; d_draws [npairs][W][4] with W = max(maxIterations, nIterations);
        d_best_inlier [npairs][cap] uint8 and d_best_pose are read and rewritten in place where given.  The parameters, the element
        types and the sizes are checked here; the arrays' contents are not read.  Returns a dict of freshly allocated tensors:
        pose_out (bytes of KF_POSE_DTYPE per pair: what PoseOptimization reads as d_pose), inlier, kp_point_out [npairs][cap],
        info [npairs][PNP_INFO], ninliers [npairs] and, with trace, trace (bytes of PNP_HYPOTHESIS_DTYPE, [npairs][W])."""
        import torch
        name = "PnPsolver.iterate_batch_device"
        W = PnPsolver.check_params(name, probability, minInliers, maxIterations, minSet, epsilon, th2, first_iteration, nIterations)
        for nm, t_ in (("d_pair_frame", d_pair_frame), ("d_n", d_n), ("d_kp_point", d_kp_point), ("d_first_iteration", d_first_iteration),
                       ("d_best_inliers_in", d_best_inliers_in)):
            if t_ is not None and t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor" % (name, nm))
        npairs, cap = int(npairs), int(cap_per_frame)
        if cap < 1 or cap > PnPsolver.MAX_N or npairs < 0 or int(npoints) < 0:
            raise ValueError("%s: cap_per_frame outside [1, %d] or a negative count" % (name, PnPsolver.MAX_N))
        if d_draws.element_size() != 4 or d_draws.numel() != npairs * W * 4 or d_kp_point.numel() != npairs * cap:
            raise ValueError("%s: d_draws must be [npairs][%d][4] of 4-byte elements and d_kp_point [npairs][cap]" % (name, W))
        nframes = int(d_n.numel())
        if (d_pair_frame is None and nframes < npairs) or (d_pair_frame is not None and int(d_pair_frame.numel()) != npairs) or \
                d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_camera.numel() * d_camera.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps and d_camera must hold one row per frame of d_n, d_pair_frame one entry per pair" % name)
        if d_points.numel() * d_points.element_size() < int(npoints) * MAP_POINT_DTYPE.itemsize or \
                (d_point_bad is not None and d_point_bad.numel() * d_point_bad.element_size() < int(npoints)):
            raise ValueError("%s: the table is shorter than npoints" % name)
        if (d_best_inlier is not None and (d_best_inlier.element_size() != 1 or d_best_inlier.numel() != npairs * cap)) or \
                (d_best_pose is not None and d_best_pose.numel() * d_best_pose.element_size() != npairs * KF_POSE_DTYPE.itemsize):
            raise ValueError("%s: d_best_inlier must be [npairs][cap] bytes and d_best_pose one pose per pair" % name)
        dev = d_kp_point.device
        prm = np.zeros(1, PNP_PARAMS_DTYPE)
        prm["probability"], prm["min_inliers"], prm["max_iterations"], prm["min_set"], prm["epsilon"], prm["th2"] = \
            probability, minInliers, maxIterations, minSet, epsilon, th2
        prm["first_iteration"], prm["niterations"], prm["best_inliers_in"] = first_iteration, nIterations, best_inliers_in
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(pose_out=e((npairs, KF_POSE_DTYPE.itemsize), torch.uint8), inlier=e((npairs, cap), torch.uint8),
                   kp_point_out=e((npairs, cap), torch.int32), info=e((npairs, PNP_INFO), torch.int32), ninliers=e((npairs,), torch.int32))
        if trace:
            out["trace"] = e((npairs, W * PNP_HYPOTHESIS_DTYPE.itemsize), torch.uint8)
        q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_pnp_solver_batch_device(
            ext._h, q(d_kps), q(d_n), cap, q(d_pair_frame), npairs, q(d_camera), q(d_kp_point), int(npoints), q(d_points), q(d_point_bad), _p(prm),
            q(d_first_iteration), q(d_best_inliers_in), q(d_draws), q(d_best_inlier), q(d_best_pose), q(out["pose_out"]), q(out["inlier"]),
            q(out["kp_point_out"]), q(out.get("trace")), q(out["info"]), q(out["ninliers"]), C.c_void_p(s)))
        return out


# pgorb_initializer: the parameter block, a traced hypothesis, the status bits, the info tables and the limit (include/pgorb.h)
INIT_PARAMS_DTYPE = np.dtype([("sigma", "<f4"), ("max_iterations", "<i4"), ("min_parallax", "<f4"), ("min_triangulated", "<i4")])
INIT_HYPOTHESIS_DTYPE = np.dtype([("H21", "<f4", (9,)), ("F21", "<f4", (9,)), ("scoreH", "<f4"), ("scoreF", "<f4"), ("inliersH", "<i4"),
                                  ("inliersF", "<i4"), ("set", "<i4", (8,))])
INIT_FEW, INIT_NO_MODEL, INIT_MODEL_H, INIT_MODEL_F, INIT_OK, INIT_DEGENERATE_H, INIT_AMBIGUOUS, INIT_FEW_GOOD, INIT_LOW_PARALLAX = \
    1, 2, 4, 8, 16, 32, 64, 128, 256
INIT_INFO, INIT_FINFO, INIT_MAX_ITERATIONS = 17, 11, 1024


def _camera_record(camera, name):
    """a KF_POSE_DTYPE record from one, or from (fx, fy, cx, cy); the four values must be finite"""
    if getattr(camera, "dtype", None) == KF_POSE_DTYPE:
        P = np.array(camera, KF_POSE_DTYPE).reshape(1)
    else:
        fx, fy, cx, cy = (np.float32(x) for x in camera)
        P = np.zeros(1, KF_POSE_DTYPE)
        with np.errstate(all="ignore"):
            P["fx"], P["fy"], P["cx"], P["cy"], P["invfx"], P["invfy"] = fx, fy, cx, cy, np.float32(1) / fx, np.float32(1) / fy
    if not np.isfinite([float(P[q][0]) for q in ("fx", "fy", "cx", "cy")]).all():
        raise ValueError("%s: the camera is not finite" % name)
    return P


class Initializer:
    """Initializer (thirdparty/orb-slam2/src/Initializer.cc) on the GPU, with the reference's surface: the constructor and
    Initialize.  ReferenceFrame / CurrentFrame: Frame-like objects (ext, N, mvKeysUndistorted: pt is read); camera: a KF_POSE_DTYPE
    record or (fx, fy, cx, cy) (mK; default ReferenceFrame.camera).  draws: [>= iterations][8] raw rand() values in [0, 2^31);
    None draws them from numpy's RandomState(seed).  After Initialize: status / info / finfo, pose (the two KF_POSE_DTYPE records of
    Tracking.cc:622-626), matches12_out (Tracking.cc:612-619) and map (the arrays pgorb_refresh_map_points and global bundle
    adjustment read: points, kf_point1, kf_point2, obs_start, obs_frame, obs_idx, npoints); trace where trace=True.
    Every input the library's checked call refuses is a ValueError here, before the library is called."""
    MAX_N = 16000

    def __init__(self, ReferenceFrame, sigma=1.0, iterations=200, draws=None, camera=None, seed=0, minParallax=1.0, minTriangulated=50):
        self.ext = ReferenceFrame.ext
        self._k1 = self.check_frame("Initializer", ReferenceFrame)
        self._cam = _camera_record(camera if camera is not None else ReferenceFrame.camera, "Initializer")
        self.check_params("Initializer", sigma, iterations, minParallax, draws)
        self.mSigma, self.mMaxIterations, self._draws_in, self._seed = float(sigma), int(iterations), draws, seed
        self._min_parallax, self._min_tri = float(minParallax), int(minTriangulated)
        self.info, self.finfo = np.zeros(INIT_INFO, np.int32), np.zeros(INIT_FINFO, np.float32)

    @staticmethod
    def check_frame(name, F):
        n = int(F.N)
        if n < 0:
            raise ValueError("%s: a negative keypoint count" % name)
        k = _arr(F.mvKeysUndistorted, KEYPOINT_DTYPE, n, name + " keypoints")
        if n and not (np.isfinite(k["x"]).all() and np.isfinite(k["y"]).all()):
            raise ValueError("%s: a keypoint coordinate is not finite" % name)
        if n > Initializer.MAX_N:
            raise ValueError("%s: more than %d keypoints in the frame" % (name, Initializer.MAX_N))
        return k

    @staticmethod
    def check_params(name, sigma, iterations, minParallax=1.0, draws=None):
        s = float(np.float32(sigma))
        if not (s > 0.0 and np.isfinite(s)) or not np.isfinite(float(np.float32(minParallax))):
            raise ValueError("%s: sigma must be positive and finite, minParallax finite" % name)
        if int(iterations) < 1:
            raise ValueError("%s: iterations is below 1" % name)
        if int(iterations) > INIT_MAX_ITERATIONS:
            raise ValueError("%s: iterations above %d" % (name, INIT_MAX_ITERATIONS))
        if draws is not None:
            d = np.asarray(draws)
            if d.ndim < 2 or d.shape[-1] != 8 or d.shape[-2] < int(iterations):
                raise ValueError("%s: draws must be [iterations][8]" % name)
            if d.size and (int(d.min()) < 0 or int(d.max()) >= 2 ** 31):
                raise ValueError("%s: a draw is not in [0, 2^31)" % name)

    def Initialize(self, CurrentFrame, vMatches12, trace=False):
        """Initializer::Initialize (:44-121).  Returns (ok, R21, t21, vP3D, vbTriangulated): R21 3 x 3 and t21 3 x 1 float32 (None
        when ok is False), vP3D [n1][3] float32, vbTriangulated [n1] bool."""
        k1, n1 = self._k1, len(self._k1)
        k2 = self.check_frame("Initialize", CurrentFrame)
        n2 = len(k2)
        m = _arr(vMatches12, np.int32, n1, "vMatches12")
        if n1 and (int(m.min()) < -1 or int(m.max()) >= n2):
            raise ValueError("Initialize: vMatches12 is outside [-1, n2)")
        it = self.mMaxIterations
        if self._draws_in is None:
            draws = np.random.RandomState(self._seed).randint(0, 2 ** 31, (it, 8)).astype(np.uint32)
        else:
            draws = np.ascontiguousarray(np.asarray(self._draws_in)[:it], np.uint32)
        prm = np.zeros(1, INIT_PARAMS_DTYPE)
        prm["sigma"], prm["max_iterations"], prm["min_parallax"], prm["min_triangulated"] = self.mSigma, it, self._min_parallax, self._min_tri
        c1, c2 = max(n1, 1), max(n2, 1)
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
        pose = np.zeros(2, KF_POSE_DTYPE)
        P3D, tri, mo = np.zeros((c1, 3), np.float32), np.zeros(c1, np.uint8), np.full(c1, -1, np.int32)
        pts, kp1, kp2 = np.zeros(c1, MAP_POINT_DTYPE), np.full(c1, -1, np.int32), np.full(c2, -1, np.int32)
        os_, of, oi, npnt = np.zeros(c1 + 1, np.int32), np.full(2 * c1, -1, np.int32), np.full(2 * c1, -1, np.int32), np.zeros(1, np.int32)
        tr = np.zeros(it, INIT_HYPOTHESIS_DTYPE) if trace else None
        info, finfo = np.zeros(INIT_INFO, np.int32), np.zeros(INIT_FINFO, np.float32)
        ext = self.ext
        ret = ext._check(ext._L.pgorb_initializer(
            ext._h, _p(pad(k1, KEYPOINT_DTYPE)), n1, _p(pad(k2, KEYPOINT_DTYPE)), n2, _p(self._cam), _p(pad(m, np.int32)), _p(prm), _p(draws),
            _p(pose), _p(P3D), _p(tri), _p(mo), _p(pts), _p(kp1), _p(kp2), _p(os_), _p(of), _p(oi), _p(npnt),
            None if tr is None else _p(tr), _p(info), _p(finfo)))
        np_ = int(npnt[0])
        self.info, self.finfo, self.status, self.trace = info, finfo, int(info[0]), tr
        self.pose, self.matches12_out, self.ntriangulated = pose, mo[:n1].copy(), int(ret)
        self.map = dict(points=pts[:np_].copy(), kf_point1=kp1[:n1].copy(), kf_point2=kp2[:n2].copy(), obs_start=os_[:np_ + 1].copy(),
                        obs_frame=of[:2 * np_].copy(), obs_idx=oi[:2 * np_].copy(), npoints=np_)
        ok = bool(info[0] & INIT_OK)
        R21 = t21 = None
        if ok:
            T = pose[1]["Tcw"].reshape(3, 4)
            R21, t21 = T[:, :3].copy(), T[:, 3:].copy()
        return ok, R21, t21, P3D[:n1].copy(), tri[:n1].astype(bool)

    @staticmethod
    def initialize_batch_device(ext, d_kps, d_n, cap_per_frame, d_pair_f1, d_pair_f2, npairs, d_camera, d_matches12, d_draws, sigma=1.0,
                                iterations=200, minParallax=1.0, minTriangulated=50, with_map=True, trace=False, stream=None):
        """pgorb_initializer_batch_device over resident torch tensors: pair p initialises from frames d_pair_f1[p] and d_pair_f2[p]
        (the layout ORBmatcher's SearchForInitialization batch writes: d_matches12 [npairs][cap]); d_camera holds one KF_POSE_DTYPE
        record per frame; d_draws [npairs][iterations][8].  The parameters, the element types and the sizes are checked here; the
        arrays' contents are not read.  Returns a dict of freshly allocated tensors: pose_out (bytes of two KF_POSE_DTYPE per pair),
        P3D [npairs][cap][3], triangulated, matches12_out [npairs][cap], info [npairs][INIT_INFO], finfo [npairs][INIT_FINFO]; with
        with_map points (bytes of MAP_POINT_DTYPE, [npairs][cap]), kf_point1, kf_point2 [npairs][cap], obs_start [npairs][cap + 1],
        obs_frame, obs_idx [npairs][2*cap], npoints [npairs]; with trace, trace (bytes of INIT_HYPOTHESIS_DTYPE, [npairs][iterations])."""
        import torch
        name = "Initializer.initialize_batch_device"
        Initializer.check_params(name, sigma, iterations, minParallax)
        it, npairs, cap = int(iterations), int(npairs), int(cap_per_frame)
        for nm, t_ in (("d_pair_f1", d_pair_f1), ("d_pair_f2", d_pair_f2), ("d_n", d_n), ("d_matches12", d_matches12)):
            if t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor" % (name, nm))
        if cap < 1 or cap > Initializer.MAX_N or npairs < 0:
            raise ValueError("%s: cap_per_frame outside [1, %d] or a negative count" % (name, Initializer.MAX_N))
        if d_draws.element_size() != 4 or d_draws.numel() != npairs * it * 8 or d_matches12.numel() != npairs * cap:
            raise ValueError("%s: d_draws must be [npairs][%d][8] of 4-byte elements and d_matches12 [npairs][cap]" % (name, it))
        nframes = int(d_n.numel())
        if int(d_pair_f1.numel()) != npairs or int(d_pair_f2.numel()) != npairs or \
                d_kps.numel() * d_kps.element_size() != nframes * cap * KEYPOINT_DTYPE.itemsize or \
                d_camera.numel() * d_camera.element_size() != nframes * KF_POSE_DTYPE.itemsize:
            raise ValueError("%s: d_kps and d_camera must hold one row per frame of d_n, d_pair_f1 / d_pair_f2 one entry per pair" % name)
        dev = d_matches12.device
        prm = np.zeros(1, INIT_PARAMS_DTYPE)
        prm["sigma"], prm["max_iterations"], prm["min_parallax"], prm["min_triangulated"] = sigma, it, minParallax, minTriangulated
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(pose_out=e((npairs, 2 * KF_POSE_DTYPE.itemsize), torch.uint8), P3D=e((npairs, cap, 3), torch.float32),
                   triangulated=e((npairs, cap), torch.uint8), matches12_out=e((npairs, cap), torch.int32),
                   info=e((npairs, INIT_INFO), torch.int32), finfo=e((npairs, INIT_FINFO), torch.float32))
        if with_map:
            out.update(points=e((npairs, cap * MAP_POINT_DTYPE.itemsize), torch.uint8), kf_point1=e((npairs, cap), torch.int32),
                       kf_point2=e((npairs, cap), torch.int32), obs_start=e((npairs, cap + 1), torch.int32),
                       obs_frame=e((npairs, 2 * cap), torch.int32), obs_idx=e((npairs, 2 * cap), torch.int32), npoints=e((npairs,), torch.int32))
        if trace:
            out["trace"] = e((npairs, it * INIT_HYPOTHESIS_DTYPE.itemsize), torch.uint8)
        q = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_initializer_batch_device(
            ext._h, q(d_kps), q(d_n), cap, q(d_pair_f1), q(d_pair_f2), npairs, q(d_camera), q(d_matches12), _p(prm), q(d_draws),
            q(out["pose_out"]), q(out["P3D"]), q(out["triangulated"]), q(out["matches12_out"]), q(out.get("points")), q(out.get("kf_point1")),
            q(out.get("kf_point2")), q(out.get("obs_start")), q(out.get("obs_frame")), q(out.get("obs_idx")), q(out.get("npoints")),
            q(out.get("trace")), q(out["info"]), q(out["finfo"]), C.c_void_p(s)))
        return out


# pgorb_refresh_map_points: what to refresh, the status word's bits, the limit (include/pgorb.h)
MP_DESCRIPTOR, MP_NORMAL_DEPTH, MP_BOTH = 1, 2, 3
MP_LIMIT, MP_BAD_INDEX, MP_MAX_OBS = -6, -1, 512


class LocalMapping:
    """LocalMapping::CreateNewMapPoints (thirdparty/orb-slam2/src/LocalMapping.cc:209-454), monocular, on the GPU."""

    @staticmethod
    def CreateNewMapPoints(KF1, neighbours, fv1, fvs, pose1, poses, median_depths, has_point1=None, has_points=None):
        """KF1 and each neighbour: a Frame-like object (ext, N, mvKeysUndistorted, mDescriptors); fv1 / fvs[s]: the (nodes,
        starts, features) triples of ORBVocabulary.transform(); pose1 / poses[s]: KF_POSE_DTYPE records (kf_pose()); median_depths[s]
        = neighbour s's ComputeSceneMedianDepth(2); has_point*[i] = GetMapPoint(i) != NULL (None = none).  Neighbours in the
        order GetBestCovisibilityKeyFrames returns them.  Returns (points, count, F12, epipole, has_point1_out): points a
        NEW_MAP_POINT_DTYPE array in the reference's creation order, count[s] the points made with neighbour s or CNM_SKIPPED,
        F12 [nneigh, 3, 3], epipole [nneigh, 2], has_point1_out KF1's mask afterwards (pgorb.h states what is left to the caller)."""
        nn = len(neighbours)
        if len(fvs) != nn or len(poses) != nn or (has_points is not None and len(has_points) != nn):
            raise ValueError("CreateNewMapPoints: neighbours, fvs, poses and has_points differ in length")
        if nn > CNM_MAX_NEIGHBOURS:
            raise ValueError("CreateNewMapPoints: more than %d neighbours" % CNM_MAX_NEIGHBOURS)
        md = _arr(median_depths, np.float32, nn, "median_depths")
        k1, d1 = _frame(KF1, "KF1")
        h1 = _mask(has_point1, KF1.N, "KF1 has_point")
        n1, s1, f1 = _featvec(fv1, "KF1")
        p1 = np.ascontiguousarray(pose1, KF_POSE_DTYPE).reshape(())
        keep = []
        kps, descs, masks, nodes, starts, feats = [(C.c_void_p * max(nn, 1))() for _ in range(6)]
        n2 = np.zeros(max(nn, 1), np.int32)
        nfv2 = np.zeros(max(nn, 1), np.int32)
        for s, K in enumerate(neighbours):
            name = "neighbour %d" % s
            kp, desc = _frame(K, name)
            m = _mask(None if has_points is None else has_points[s], K.N, name + " has_point")
            node, start, feat = _featvec(fvs[s], name)
            keep += [kp, desc, m, node, start, feat]
            kps[s], descs[s], masks[s], nodes[s], starts[s], feats[s] = (a.ctypes.data for a in (kp, desc, m, node, start, feat))
            n2[s], nfv2[s] = K.N, len(node)
        P2 = np.zeros(max(nn, 1), KF_POSE_DTYPE)
        for s in range(nn):
            P2[s] = np.asarray(poses[s], KF_POSE_DTYPE).reshape(())
        ext = KF1.ext
        pts = np.zeros(max(KF1.N, 1), NEW_MAP_POINT_DTYPE)
        count = np.zeros(max(nn, 1), np.int32)
        F12 = np.zeros((max(nn, 1), 9), np.float32)
        ep = np.zeros((max(nn, 1), 2), np.float32)
        hout = np.zeros(max(KF1.N, 1), np.uint8)
        np_ = ext._check(ext._L.pgorb_create_new_map_points(
            ext._h, _p(k1), _p(d1), _p(h1), KF1.N, _p(n1), _p(s1), _p(f1), len(n1), _p(p1), nn, kps, descs, masks, _p(n2), nodes,
            starts, feats, _p(nfv2), _p(P2), _p(md), _p(pts), _p(count), _p(F12), _p(ep), _p(hout)))
        return pts[:np_].copy(), count[:nn].copy(), F12[:nn].reshape(nn, 3, 3).copy(), ep[:nn].copy(), hout[:KF1.N].copy()


    @staticmethod
    def RefreshMapPoints(key_frames, poses, points, descriptors, obs_start, obs_frame, obs_idx, ref_obs=None, point_bad=None,
                         kf_bad=None, select=None, what=MP_BOTH, ext=None):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:259-324) and MapPoint::UpdateNormalAndDepth (:347-388) of many
        points in one call, as LocalMapping.cc:444-446 and :519-532 run them.  key_frames: Frame-like objects (ext, N,
        mvKeysUndistorted, mDescriptors); poses[f]: KF_POSE_DTYPE; kf_bad[f] = isBad() (None = none).  points (MAP_POINT_DTYPE),
        descriptors [n, 32], point_bad (None = none); point i observes (obs_frame[k], obs_idx[k]) = (position in key_frames,
        keypoint) for k in obs_start[i]:obs_start[i + 1], IN THE ORDER mObservations ITERATES (include/pgorb.h); ref_obs[i] = the
        position of mpRefKF in that list.  select: table indices (None = all); what: MP_DESCRIPTOR | MP_NORMAL_DEPTH | MP_BOTH.
        Returns (points, descriptors, best_obs, status): copies with the refreshed fields, and per selected point the winning
        observation's list position (-1: descriptor unchanged) and the status word (bits MP_DESCRIPTOR / MP_NORMAL_DEPTH, or
        MP_LIMIT for a list longer than MP_MAX_OBS).  Raises ValueError for everything pgorb_refresh_map_points refuses."""
        fn = "RefreshMapPoints"
        nkf = len(key_frames)
        if ext is None:
            if not nkf:
                raise ValueError(fn + ": no key frame and no ext")
            ext = key_frames[0].ext
        if what not in (MP_DESCRIPTOR, MP_NORMAL_DEPTH, MP_BOTH):
            raise ValueError(fn + ": what must be MP_DESCRIPTOR, MP_NORMAL_DEPTH or MP_BOTH")
        if len(poses) != nkf:
            raise ValueError(fn + ": key_frames and poses differ in length")
        P = np.zeros(max(nkf, 1), KF_POSE_DTYPE)
        keep = []
        kps, descs = [(C.c_void_p * max(nkf, 1))() for _ in range(2)]
        nk = np.zeros(max(nkf, 1), np.int32)
        for f, K in enumerate(key_frames):
            kp, d = _frame(K, "key frame %d" % f)
            keep += [kp, d]
            kps[f], descs[f], nk[f] = kp.ctypes.data, d.ctypes.data, K.N
            P[f] = np.asarray(poses[f], KF_POSE_DTYPE).reshape(())
        kb = _mask(kf_bad, nkf, "kf_bad")
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))       # a copy: refreshed in place
        n = len(pts)
        pd = np.array(_arr(descriptors, np.uint8, n, "point descriptors", 32))
        pb = _mask(point_bad, n, "point_bad")
        st = _arr(obs_start, np.int32, n + 1, "obs_start")
        of = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
        oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
        if st[0] != 0 or np.any(np.diff(st) < 0) or len(of) < int(st[-1]) or len(oi) < int(st[-1]):
            raise ValueError(fn + ": obs_start must rise from 0 to at most len(obs_frame), len(obs_idx)")
        m = int(st[-1])
        if m and (of[:m].min() < 0 or of[:m].max() >= nkf or oi[:m].min() < 0 or np.any(oi[:m] >= nk[np.clip(of[:m], 0, max(nkf - 1, 0))])):
            raise ValueError(fn + ": an observation names a key frame or keypoint out of range")
        owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(st))
        pair = owner * max(nkf, 1) + of[:m]
        if len(np.unique(pair)) != m:
            raise ValueError(fn + ": a list names a key frame twice")
        if select is None:
            sel, nsel = None, n
            chosen = np.arange(n)
        else:
            sel = np.ascontiguousarray(select, np.int32).reshape(-1)
            nsel = len(sel)
            if nsel and (sel.min() < 0 or sel.max() >= n):
                raise ValueError(fn + ": a selection index is out of range")
            if len(np.unique(sel)) != nsel:
                raise ValueError(fn + ": a point is selected twice")
            chosen = sel
        if what & MP_NORMAL_DEPTH:
            ro = _arr(ref_obs if ref_obs is not None else [], np.int32, n, "ref_obs")
            ln = np.diff(st)[chosen]
            need = (pb[:n][chosen] == 0) & (ln > 0) & (ln <= MP_MAX_OBS)
            if np.any(need & ((ro[chosen] < 0) | (ro[chosen] >= ln))):
                raise ValueError(fn + ": ref_obs lies outside the point's list")
        else:
            ro = np.zeros(max(n, 1), np.int32) if ref_obs is None else _arr(ref_obs, np.int32, n, "ref_obs")
        if len(of) == 0:
            of, oi = np.zeros(1, np.int32), np.zeros(1, np.int32)
        if len(ro) == 0:
            ro = np.zeros(1, np.int32)
        best = np.full(max(nsel, 1), -1, np.int32)
        status = np.zeros(max(nsel, 1), np.int32)
        pts_buf = pts if n else np.zeros(1, MAP_POINT_DTYPE)
        pd_buf = pd if n else np.zeros((1, 32), np.uint8)
        ext._check(ext._L.pgorb_refresh_map_points(ext._h, nkf, kps, descs, _p(nk), _p(P), _p(kb), n, _p(pts_buf), _p(pd_buf), _p(pb),
                                                   _p(st), _p(of), _p(oi), _p(ro), nsel, None if sel is None else _p(sel if nsel else best),
                                                   int(what), _p(best), _p(status)))
        return pts, pd, best[:nsel].copy(), status[:nsel].copy()

    @staticmethod
    def MapPointCulling(ext, kf_point, npoints, point_bad, obs_start, obs_frame, obs_idx, obs_live, first_kf_id, visible, found, recent,
                        cur_kf_id, th_obs=2):
        """LocalMapping::MapPointCulling (src/LocalMapping.cc:170-207) over recent = mlpRecentAddedMapPoints as table indices.
        kf_point[f] = key frame f's slots; the table's lists as CSR with the mask obs_live; first_kf_id / visible / found per
        point.  Nothing passed in is changed.  Returns a dict: kf_point (a list of arrays), point_bad, obs_live afterwards, action
        [nrecent] (CULL_MP_*), recent (the surviving list) and info.  Raises ValueError for everything pgorb_map_point_culling refuses."""
        fn = "LocalMapping.MapPointCulling"
        n, nkf = int(npoints), len(kf_point)
        slots, ptrs, nk, st, of, oi, live, pb = _cull_table(fn, nkf, kf_point, n, point_bad, obs_start, obs_frame, obs_idx, obs_live, None)[:8]
        fk, vi, fo = (_arr(x, np.int32, n, nm) for x, nm in ((first_kf_id, "first_kf_id"), (visible, "visible"), (found, "found")))
        rec = np.ascontiguousarray(recent, np.int32).reshape(-1)
        if len(rec) and (rec.min() < 0 or rec.max() >= n):
            raise ValueError(fn + ": a recent entry is out of range")
        if len(np.unique(rec)) != len(rec):
            raise ValueError(fn + ": the recent list names a point twice")
        nr = max(len(rec), 1)
        action, out, nout, info = np.zeros(nr, np.int32), np.zeros(nr, np.int32), np.zeros(1, np.int32), np.zeros(CULL_INFO, np.int32)
        one = np.zeros(1, np.int32)
        ext._check(ext._L.pgorb_map_point_culling(
            ext._h, nkf, ptrs, _p(nk), n, _p(pb), _p(st), _p(of), _p(oi), _p(live), _p(fk if n else one), _p(vi if n else one), _p(fo if n else one),
            len(rec), _p(rec if len(rec) else one), int(cur_kf_id), int(th_obs), _p(action), _p(out), _p(nout), _p(info)))
        return dict(kf_point=slots, point_bad=pb[:n], obs_live=live[:int(st[-1])], action=action[:len(rec)], recent=out[:int(nout[0])].copy(), info=info)

    @staticmethod
    def KeyFrameCulling(graph, cur_kf, octaves, kf_point, npoints, point_bad, obs_start, obs_frame, obs_idx, obs_live, ref_obs, kf_bad=None,
                        kf_not_erase=None, kf_to_be_erased=None, list_cap=None):
        """LocalMapping::KeyFrameCulling (src/LocalMapping.cc:634-698) with KeyFrame::SetBadFlag and MapPoint::EraseObservation over
        `graph` (a CovisibilityGraph, updated IN PLACE) with mpCurrentKeyFrame = cur_kf.  octaves[f] = mvKeysUn[i].octave of key
        frame f, kf_point[f] its slots; the table's lists as CSR with the mask obs_live and ref_obs.  Apart from the graph nothing
        passed in is changed.  Returns a dict: kf_point, point_bad, obs_live, ref_obs, kf_bad, kf_to_be_erased afterwards, record
        [list length][4] = (key frame, nMPs, nRedundantObservations, CULL_KF_*), row_status (CULL_ROW_*) and info; info[0] ==
        CULL_LIMIT: the list is longer than list_cap (default: conn_cap) and nothing was done.  Raises ValueError for everything
        pgorb_keyframe_culling refuses."""
        fn = "LocalMapping.KeyFrameCulling"
        n, nkf = int(npoints), graph.nkf
        slots, ptrs, nk, st, of, oi, live, pb, ko = _cull_table(fn, nkf, kf_point, n, point_bad, obs_start, obs_frame, obs_idx, obs_live, graph.kf_order)
        if not 0 <= int(cur_kf) < nkf:
            raise ValueError(fn + ": cur_kf is out of range")
        list_cap = graph.conn_cap if list_cap is None else int(list_cap)
        if list_cap < 1:
            raise ValueError(fn + ": list_cap < 1")
        if len(octaves) != nkf or any(len(o) != len(s) for o, s in zip(octaves, slots)):
            raise ValueError(fn + ": one octave per slot of every key frame")
        ro = np.array(_arr(ref_obs, np.int32, n, "ref_obs"))
        ln = np.diff(st)
        if np.any((ln > 0) & ((ro[:n] < -1) | (ro[:n] >= ln))):
            raise ValueError(fn + ": ref_obs lies outside the point's list")
        _covis_rows(fn, graph, nkf, ko)
        keep = []
        kps = (C.c_void_p * max(nkf, 1))()
        for f, o in enumerate(octaves):
            k = np.zeros(max(len(o), 1), KEYPOINT_DTYPE)
            k["octave"][:len(o)] = o
            keep.append(k)
            kps[f] = k.ctypes.data
        kb, ne, tbe = (np.array(_mask(m, nkf, nm)) for m, nm in ((kf_bad, "kf_bad"), (kf_not_erase, "kf_not_erase"), (kf_to_be_erased, "kf_to_be_erased")))
        record, status, info = np.zeros((list_cap, 4), np.int32), np.zeros(max(nkf, 1), np.int32), np.zeros(CULL_INFO, np.int32)
        ext = graph.ext
        ext._check(ext._L.pgorb_keyframe_culling(
            ext._h, nkf, kps, ptrs, _p(nk), n, _p(pb), _p(st), _p(of), _p(oi), _p(live), _p(ro if n else np.zeros(1, np.int32)),
            None if ko is None else _p(ko), _p(graph.kf_id0), _p(ne), _p(kb), _p(tbe), int(cur_kf), graph.conn_cap, _p(graph.conn_kf), _p(graph.conn_w),
            _p(graph.nconn), _p(graph.ord_kf), _p(graph.ord_w), _p(graph.nord), _p(graph.parent), list_cap, _p(record), _p(status), _p(info)))
        nl = 0 if info[0] & CULL_LIMIT else int(info[1])
        return dict(kf_point=slots, point_bad=pb[:n], obs_live=live[:int(st[-1])], ref_obs=ro[:n], kf_bad=kb[:nkf], kf_to_be_erased=tbe[:nkf],
                    record=record[:nl].copy(), row_status=status[:nkf].copy(), info=info)

    @staticmethod
    def ProcessNewKeyFrame(ext, kf, kf_point, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live, ref_obs,
                           kf_order=None):
        """LocalMapping::ProcessNewKeyFrame's AddObservation loop (src/LocalMapping.cc:142-161) for key frame kf, as map edits
        (map_edit.process_new_key_frame): the dict of apply_map_edits with slot_class added."""
        from .map_edit import process_new_key_frame
        return process_new_key_frame(ext, kf, kf_point, npoints, point_bad, visible, found, replaced, obs_start, obs_frame, obs_idx, obs_live,
                                     ref_obs, kf_order)

    @staticmethod
    def KeyFrameTcp(ext, poses, parent, record, tcp=None):
        """KeyFrame::SetBadFlag's mTcp = Tcw * mpParent->GetPoseInverse() (src/KeyFrame.cc:641) for every row of `record`
        (KeyFrameCulling's, [m][4]) whose action is CULL_KF_CULLED; poses / parent as they stand right after that culling, before any
        call that moves a pose.  tcp [nkf][12] = the rows so far (None = zeros); a copy is updated.  Returns a dict: tcp, info
        [TCP_INFO] = (0, written, skipped), written.  Raises ValueError for everything pgorb_keyframe_tcp refuses."""
        fn = "LocalMapping.KeyFrameTcp"
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        nkf = len(par)
        rec = np.ascontiguousarray(record, np.int32).reshape(-1, 4)
        if nkf > COVIS_MAX_KF or len(rec) > COVIS_MAX_KF:
            raise ValueError(fn + ": more than COVIS_MAX_KF key frames or records")
        P = np.ascontiguousarray(poses, KF_POSE_DTYPE).reshape(-1)
        if len(P) != nkf:
            raise ValueError(fn + ": one pose per key frame")
        out = np.zeros((max(nkf, 1), 12), np.float32)
        if tcp is not None:
            out[:nkf] = _arr(tcp, np.float32, nkf, "tcp", 12)
        info = np.zeros(TCP_INFO, np.int32)
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
        ret = ext._check(ext._L.pgorb_keyframe_tcp(ext._h, nkf, _p(pad(P, KF_POSE_DTYPE)), _p(pad(par, np.int32)), len(rec),
                                                   _p(rec if len(rec) else np.zeros((1, 4), np.int32)), _p(out), _p(info)))
        return dict(tcp=out[:nkf].copy(), info=info, written=int(ret))

    @staticmethod
    def _depth_table(fn, kf_point, n, poses, points):
        """(kf_point [nframes][cap], n, poses, points, npoints), checked as pgorb_scene_median_depth checks them"""
        kfp = np.ascontiguousarray(kf_point, np.int32)
        if kfp.ndim != 2 or kfp.shape[0] > COVIS_MAX_KF or kfp.shape[1] > 16000:
            raise ValueError(fn + ": kf_point is [nframes][cap_per_frame], at most COVIS_MAX_KF frames of 16000 keypoints")
        nframes, cap = kfp.shape
        nn = _arr(n, np.int32, nframes, fn + " n")
        P = _arr(poses, KF_POSE_DTYPE, nframes, fn + " poses")
        X = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
        if nframes and (nn.min() < 0 or nn.max() > cap):
            raise ValueError(fn + ": a frame's count is outside [0, cap_per_frame]")
        for f in range(nframes):
            u = kfp[f, :nn[f]]
            if len(u) and (u.min() < -1 or u.max() >= len(X)):
                raise ValueError(fn + ": a slot names a point out of range")
        return kfp, nn, P, X, len(X)

    @staticmethod
    def SceneMedianDepth(ext, kf_list, q, kf_point, n, poses, points):
        """KeyFrame::ComputeSceneMedianDepth(q) (src/KeyFrame.cc:736-766) for every key frame of kf_list (-1 = skipped: its entries
        come back as 0 / 0).  Returns (median float32 [nlist], status int32 [nlist]): -1 with DEPTH_EMPTY for a key frame without
        points, -1 with DEPTH_NAN when a depth is NaN.  The medians of a key frame's neighbours are what CreateNewMapPoints takes as
        median_depths.  Raises ValueError for what pgorb_scene_median_depth refuses."""
        fn = "LocalMapping.SceneMedianDepth"
        kfp, nn, P, X, npoints = LocalMapping._depth_table(fn, kf_point, n, poses, points)
        lst = np.ascontiguousarray(kf_list, np.int32).reshape(-1)
        if int(q) < 1 or len(lst) > DEPTH_MAX_LIST or (len(lst) and (lst.min() < -1 or lst.max() >= len(kfp))):
            raise ValueError(fn + ": q < 1, more than DEPTH_MAX_LIST entries, or a key frame out of range")
        med, st = np.zeros(max(len(lst), 1), np.float32), np.zeros(max(len(lst), 1), np.int32)
        pad = lambda x, dt: x if len(x) else np.zeros(1, dt)
        ext._check(ext._L.pgorb_scene_median_depth(ext._h, len(lst), _p(pad(lst, np.int32)), int(q), _p(pad(kfp.reshape(-1), np.int32)),
                                                   _p(pad(nn, np.int32)), kfp.shape[0], kfp.shape[1], _p(pad(P, KF_POSE_DTYPE)), npoints,
                                                   _p(pad(X, MAP_POINT_DTYPE)), _p(med), _p(st)))
        return med[:len(lst)], st[:len(lst)]


# the cullings (include/pgorb.h): MapPointCulling's and KeyFrameCulling's action codes, the row status bits
CULL_MP_KEEP, CULL_MP_WAS_BAD, CULL_MP_FOUND_RATIO, CULL_MP_FEW_OBS, CULL_MP_AGED, CULL_MP_NONE = 0, 1, 2, 3, 4, 5
CULL_KF_KEEP, CULL_KF_CULLED, CULL_KF_TO_BE_ERASED, CULL_KF_ID0, CULL_KF_WAS_BAD, CULL_KF_NONE = 0, 1, 2, 3, 4, 5
CULL_ROW_ERASED, CULL_ROW_CLEARED, CULL_ROW_REPARENTED = 1, 2, 4
CULL_LIMIT, CULL_INFO = 32, 4


def _cull_table(fn, nkf, kf_point, npoints, point_bad, obs_start, obs_frame, obs_idx, obs_live, kf_order):
    """The slots and the masked observation lists as the cullings take them, checked as the single calls check them; the arrays
    that the call writes are copies."""
    slots, ptrs, nk, st, of, pb, ko = _covis_table(fn, nkf, kf_point, npoints, obs_start, obs_frame, point_bad, kf_order)
    slots = [np.array(s) for s in slots]
    for f, s in enumerate(slots):
        ptrs[f] = s.ctypes.data if len(s) else None
    m = int(st[-1])
    oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
    live = np.array(np.ascontiguousarray(obs_live, np.uint8).reshape(-1))
    if len(oi) < m or len(live) < m:
        raise ValueError(fn + ": obs_idx and obs_live need one entry per observation")
    if m and (oi[:m].min() < 0 or np.any(oi[:m] >= nk[of[:m]])):
        raise ValueError(fn + ": an observation names a keypoint out of range")
    if len(oi) == 0:
        oi, live = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    return slots, ptrs, nk, st, of, oi, live, np.array(pb), ko


def _covis_rows(fn, graph, nkf, ko):
    """The graph rows as pgorb_update_connections and pgorb_keyframe_culling require them."""
    rank = ko if ko is not None else np.arange(nkf, dtype=np.int32)
    for f in range(nkf):
        nc, no = int(graph.nconn[f]), int(graph.nord[f])
        if not (0 <= nc <= graph.conn_cap and 0 <= no <= graph.conn_cap):
            raise ValueError(fn + ": a row count is outside [0, conn_cap]")
        row = graph.conn_kf[f, :nc]
        if nc and (row.min() < 0 or row.max() >= nkf or np.any(row == f) or np.any(np.diff(rank[row]) <= 0)):
            raise ValueError(fn + ": a connection row is out of range or not in address order")
        if no and not np.all(np.isin(graph.ord_kf[f, :no], row)):
            raise ValueError(fn + ": an ordered entry is not in the row's map")
        if not -1 <= int(graph.parent[f]) < nkf:
            raise ValueError(fn + ": a parent is out of range")


def compact_observations(obs_start, obs_frame, obs_idx, obs_live, ref_obs, out=None):
    """What pgorb_compact_observations_device writes, in numpy: (obs_start, obs_frame, obs_idx, ref_obs) of the live entries, the
    order inside each list kept, ref_obs re-based (-1 when it names no live entry).  out = four arrays to fill instead (obs_frame /
    obs_idx with room for the old length); they must not share memory with an input."""
    st = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
    n = len(st) - 1
    if n < 0 or st[0] != 0 or np.any(np.diff(st) < 0):
        raise ValueError("compact_observations: obs_start must rise from 0")
    m = int(st[-1])
    of, oi, lv = (np.asarray(x).reshape(-1) for x in (obs_frame, obs_idx, obs_live))
    ro = _arr(ref_obs, np.int32, n, "ref_obs")
    if min(len(of), len(oi), len(lv)) < m:
        raise ValueError("compact_observations: obs_frame, obs_idx and obs_live need one entry per observation")
    if out is not None and any(np.shares_memory(o, i) for o in out for i in (obs_start, obs_frame, obs_idx, obs_live, ref_obs) if isinstance(i, np.ndarray)):
        raise ValueError("compact_observations: an output aliases an input")
    keep = lv[:m] != 0
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int32)           # live entries in front of each position
    start = before[st]
    pos = st[:-1].astype(np.int64) + ro
    named = (ro >= 0) & (ro < np.diff(st))
    named[named] = keep[pos[named]]
    ref = np.where(named, before[np.where(named, pos, 0)] - start[:-1], -1).astype(np.int32)
    res = (start, of[:m][keep].astype(np.int32), oi[:m][keep].astype(np.int32), ref)
    if out is None:
        return res
    for o, r in zip(out, res):
        o[:len(r)] = r
    return tuple(out)


# the covisibility graph (include/pgorb.h): row status bits, limits, the local map's status bits
COVIS_UPDATED, COVIS_RESORTED, COVIS_EMPTY, COVIS_FALLBACK, COVIS_PARENT_SET, COVIS_LIMIT = 1, 2, 4, 8, 16, 32
COVIS_MAX_KF, COVIS_MAX_CONN, COVIS_INFO = 4096, 2048, 4
LOCALMAP_NO_VOTES, LOCALMAP_LIMIT = 1, 2


def _covis_table(fn, nkf, kf_point, npoints, obs_start, obs_frame, point_bad, kf_order):
    """The slots, the observation lists and the address ranks, checked as the single calls check them."""
    if len(kf_point) != nkf:
        raise ValueError(fn + ": one slot array per key frame")
    if nkf > COVIS_MAX_KF:
        raise ValueError(fn + ": more than COVIS_MAX_KF key frames")
    slots = [np.ascontiguousarray(s, np.int32).reshape(-1) for s in kf_point]
    for s in slots:
        if len(s) > 16000:
            raise ValueError(fn + ": more than 16000 keypoints")
        if len(s) and (s.min() < -1 or s.max() >= npoints):
            raise ValueError(fn + ": a slot names a point out of range")
    st = _arr(obs_start, np.int32, npoints + 1, "obs_start")
    of = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
    if st[0] != 0 or np.any(np.diff(st) < 0) or len(of) < int(st[-1]):
        raise ValueError(fn + ": obs_start must rise from 0 to at most len(obs_frame)")
    m = int(st[-1])
    if m and (of[:m].min() < 0 or of[:m].max() >= nkf):
        raise ValueError(fn + ": an observation names a key frame out of range")
    owner = np.repeat(np.arange(npoints, dtype=np.int64), np.diff(st))
    if len(np.unique(owner * max(nkf, 1) + of[:m])) != m:
        raise ValueError(fn + ": a list names a key frame twice")
    pb = _mask(point_bad, npoints, "point_bad")
    ko = None
    if kf_order is not None:
        ko = _arr(kf_order, np.int32, nkf, "kf_order")
        if not np.array_equal(np.sort(ko), np.arange(nkf)):
            raise ValueError(fn + ": kf_order is not a permutation")
    if len(of) == 0:
        of = np.zeros(1, np.int32)
    ptrs = (C.c_void_p * max(nkf, 1))()
    for f, s in enumerate(slots):
        ptrs[f] = s.ctypes.data if len(s) else None
    nk = np.array([len(s) for s in slots] + ([0] if not nkf else []), np.int32)
    return slots, ptrs, nk, st, of, pb, ko


class CovisibilityGraph:
    """The covisibility graph of nkf key frames as the arrays the library keeps (include/pgorb.h): conn_kf / conn_w / nconn =
    mConnectedKeyFrameWeights in address order, ord_kf / ord_w / nord = mvpOrderedConnectedKeyFrames / mvOrderedWeights, parent
    (-1 = none) and first_connection.  kf_order[f] = the rank of key frame f's address (None = index order)."""

    def __init__(self, ext, nkf, conn_cap, kf_order=None, kf_id0=None):
        if conn_cap < 1 or conn_cap > COVIS_MAX_CONN:
            raise ValueError("CovisibilityGraph: conn_cap outside 1..COVIS_MAX_CONN")
        if nkf < 0 or nkf > COVIS_MAX_KF:
            raise ValueError("CovisibilityGraph: nkf outside 0..COVIS_MAX_KF")
        self.ext, self.nkf, self.conn_cap = ext, int(nkf), int(conn_cap)
        self.kf_order = None if kf_order is None else _arr(kf_order, np.int32, nkf, "kf_order")
        self.kf_id0 = _mask(kf_id0, nkf, "kf_id0")
        k1 = max(nkf, 1)
        self.conn_kf, self.conn_w = np.full((k1, conn_cap), -1, np.int32), np.zeros((k1, conn_cap), np.int32)
        self.ord_kf, self.ord_w = np.full((k1, conn_cap), -1, np.int32), np.zeros((k1, conn_cap), np.int32)
        self.nconn, self.nord = np.zeros(k1, np.int32), np.zeros(k1, np.int32)
        self.parent, self.first_connection = np.full(k1, -1, np.int32), np.ones(k1, np.uint8)

    def UpdateConnections(self, kf_point, npoints, obs_start, obs_frame, key_frames, point_bad=None, th=15, loop_conn_cap=0):
        """KeyFrame::UpdateConnections() (src/KeyFrame.cc:392-482) of `key_frames` one after another, in place.  kf_point[f] = the
        table indices of key frame f's slots (-1 = none); the table's observation lists as CSR.  Returns (row_status [nkf],
        loop_conn [m][3], info): loop_conn = LoopConnections (LoopClosing.cc:548-566) when loop_conn_cap > 0.  Raises ValueError for
        everything pgorb_update_connections refuses."""
        fn = "CovisibilityGraph.UpdateConnections"
        nkf = self.nkf
        slots, ptrs, nk, st, of, pb, ko = _covis_table(fn, nkf, kf_point, int(npoints), obs_start, obs_frame, point_bad, self.kf_order)
        lst = np.ascontiguousarray(key_frames, np.int32).reshape(-1)
        if int(th) < 1 or int(loop_conn_cap) < 0:
            raise ValueError(fn + ": th < 1 or loop_conn_cap < 0")
        if len(lst) and (lst.min() < 0 or lst.max() >= nkf):
            raise ValueError(fn + ": a list entry is out of range")
        if len(np.unique(lst)) != len(lst):
            raise ValueError(fn + ": the list names a key frame twice")
        rank = ko if ko is not None else np.arange(nkf, dtype=np.int32)
        for f in range(nkf):
            nc, no = int(self.nconn[f]), int(self.nord[f])
            if not (0 <= nc <= self.conn_cap and 0 <= no <= self.conn_cap):
                raise ValueError(fn + ": a row count is outside [0, conn_cap]")
            row = self.conn_kf[f, :nc]
            if nc and (row.min() < 0 or row.max() >= nkf or np.any(row == f) or np.any(np.diff(rank[row]) <= 0)):
                raise ValueError(fn + ": a connection row is out of range or not in address order")
            if no and not np.all(np.isin(self.ord_kf[f, :no], row)):
                raise ValueError(fn + ": an ordered entry is not in the row's map")
            if not -1 <= int(self.parent[f]) < nkf:
                raise ValueError(fn + ": a parent is out of range")
        status = np.zeros(max(nkf, 1), np.int32)
        loop = np.zeros((max(int(loop_conn_cap), 1), 3), np.int32)
        info = np.zeros(COVIS_INFO, np.int32)
        ext = self.ext
        ext._check(ext._L.pgorb_update_connections(
            ext._h, nkf, ptrs, _p(nk), int(npoints), _p(pb), _p(st), _p(of), None if ko is None else _p(ko), _p(self.kf_id0), len(lst),
            _p(lst if len(lst) else np.zeros(1, np.int32)), int(th), self.conn_cap, _p(self.conn_kf), _p(self.conn_w), _p(self.nconn),
            _p(self.ord_kf), _p(self.ord_w), _p(self.nord), _p(self.parent), _p(self.first_connection), _p(status), int(loop_conn_cap),
            _p(loop) if loop_conn_cap else None, _p(info)))
        m = 0 if info[0] & COVIS_LIMIT else min(int(info[1]), int(loop_conn_cap))
        return status[:nkf].copy(), loop[:m].copy(), info

    def GetBestCovisibilityKeyFrames(self, f, N):
        return self.ord_kf[f, :min(int(self.nord[f]), N)].copy()

    def GetCovisiblesByWeight(self, f, w):
        """KeyFrame.cc:287-302: upper_bound with weightComp; no weight below w -> an empty vector."""
        ws = self.ord_w[f, :int(self.nord[f])]
        n = int((ws >= w).sum())
        return self.ord_kf[f, :0 if n == len(ws) else n].copy()


class Tracking:
    """Tracking::UpdateLocalMap (thirdparty/orb-slam2/src/Tracking.cc:1186-1321) on the GPU."""

    @staticmethod
    def UpdateLocalMap(graph, kp_point, kf_point, npoints, obs_start, obs_frame, point_bad=None, kf_bad=None, prev_local_kf=None,
                       nbest=10, max_local=80, lkf_cap=256, qcap=16000):
        """UpdateLocalKeyFrames + UpdateLocalPoints for a frame whose mvpMapPoints are the table indices kp_point (-1 = none), over
        `graph` (a CovisibilityGraph) and the key frames' slots kf_point.  prev_local_kf = mvpLocalKeyFrames before the call (None =
        none), walked again when no point votes.  Returns a dict: kp_point (a bad point's slot cleared), local_kf, ref_kf (-1 =
        keep), queries (mvpLocalMapPoints as table indices, what SearchLocalPoints takes), status (LOCALMAP_NO_VOTES |
        LOCALMAP_LIMIT).  Raises ValueError for everything pgorb_update_local_map refuses."""
        fn = "Tracking.UpdateLocalMap"
        nkf = graph.nkf
        if nkf + 1 > COVIS_MAX_KF:
            raise ValueError(fn + ": more than COVIS_MAX_KF - 1 key frames")
        slots, ptrs, nk, st, of, pb, ko = _covis_table(fn, nkf, kf_point, int(npoints), obs_start, obs_frame, point_bad, graph.kf_order)
        kp = np.ascontiguousarray(kp_point, np.int32).reshape(-1)
        if len(kp) > 16000 or (len(kp) and (kp.min() < -1 or kp.max() >= npoints)):
            raise ValueError(fn + ": more than 16000 slots, or a slot names a point out of range")
        if not (1 <= int(lkf_cap) <= COVIS_MAX_KF and 1 <= int(qcap) <= 16000) or nbest < 0 or max_local < 0:
            raise ValueError(fn + ": lkf_cap outside 1..COVIS_MAX_KF, qcap outside 1..16000, or a negative nbest / max_local")
        prev = None if prev_local_kf is None else np.ascontiguousarray(prev_local_kf, np.int32).reshape(-1)
        if prev is not None and (len(prev) > lkf_cap or (len(prev) and (prev.min() < 0 or prev.max() >= nkf))):
            raise ValueError(fn + ": the previous list is longer than lkf_cap or names a key frame out of range")
        for f in range(nkf):
            no = int(graph.nord[f])
            if not 0 <= no <= graph.conn_cap or (no and (graph.ord_kf[f, :no].min() < 0 or graph.ord_kf[f, :no].max() >= nkf)) or \
                    not -1 <= int(graph.parent[f]) < nkf:
                raise ValueError(fn + ": an ordered row or a parent is out of range")
        kb = _mask(kf_bad, nkf, "kf_bad")
        kpo = np.zeros(max(len(kp), 1), np.int32)
        lk, q = np.zeros(int(lkf_cap), np.int32), np.zeros(int(qcap), np.int32)
        outs = [np.zeros(1, np.int32) for _ in range(4)]                  # nlocal_kf, ref_kf, nq, status
        ext = graph.ext
        ext._check(ext._L.pgorb_update_local_map(
            ext._h, nkf, ptrs, _p(nk), _p(kb), _p(kp if len(kp) else kpo), len(kp), int(npoints), _p(pb), _p(st), _p(of), graph.conn_cap,
            _p(graph.ord_kf), _p(graph.nord), _p(graph.parent), None if ko is None else _p(ko), int(nbest), int(max_local),
            -1 if prev is None else len(prev), None if prev is None or not len(prev) else _p(prev), _p(kpo), int(lkf_cap), _p(lk), _p(outs[0]),
            _p(outs[1]), int(qcap), _p(q), _p(outs[2]), _p(outs[3])))
        return dict(kp_point=kpo[:len(kp)].copy(), local_kf=lk[:int(outs[0][0])].copy(), ref_kf=int(outs[1][0]), queries=q[:int(outs[2][0])].copy(),
                    status=int(outs[3][0]))

    @staticmethod
    def _kf_poses(fn, kf_poses):
        P = np.ascontiguousarray(kf_poses, KF_POSE_DTYPE).reshape(-1)
        if len(P) > COVIS_MAX_KF:
            raise ValueError(fn + ": more than COVIS_MAX_KF key frames")
        return P, (P if len(P) else np.zeros(1, KF_POSE_DTYPE))

    @staticmethod
    def PredictPose(ext, state, mode, kf_poses, last_record=None):
        """The pose the first search of a frame starts from (Tracking.cc:792-798 + :866, or :764).  state = a TRACK_STATE_DTYPE
        record, mode = TRACK_MOTION_MODEL (UpdateLastFrame from last_record = mlTrajectory.back() and the key-frame poses, then
        mVelocity * mLastFrame.mTcw) or TRACK_REFERENCE_KF (mLastFrame.mTcw).  Nothing passed in is changed.  Returns a dict: pose
        (a complete KF_POSE_DTYPE record), state (afterwards), status (TRACK_NO_LAST | TRACK_NO_VELOCITY | TRACK_BAD_INDEX; with
        one the pose is the state's last pose and the state is unchanged).  Raises ValueError for what pgorb_track_predict refuses."""
        fn = "Tracking.PredictPose"
        if int(mode) not in (TRACK_MOTION_MODEL, TRACK_REFERENCE_KF):
            raise ValueError(fn + ": an unknown mode")
        P, Pp = Tracking._kf_poses(fn, kf_poses)
        st = np.array(np.ascontiguousarray(state, TRACK_STATE_DTYPE).reshape(()))
        rec = None if last_record is None else np.ascontiguousarray(last_record, TRAJECTORY_RECORD_DTYPE).reshape(())
        out = np.zeros((), KF_POSE_DTYPE)
        status = ext._check(ext._L.pgorb_track_predict(ext._h, int(mode), _p(st), None if rec is None else _p(rec), len(P), _p(Pp), _p(out)))
        return dict(pose=out, state=st, status=int(status))

    @staticmethod
    def CommitFrame(ext, state, pose, ok, ref_kf, frame_time, frame_id, kf_poses, trajectory, ntrajectory):
        """The end of Tracking::Track (Tracking.cc:432-440, :493, :497-506): the motion model, the trajectory record appended at
        trajectory[ntrajectory] (a TRAJECTORY_RECORD_DTYPE array, its length is the capacity) and mLastFrame.  Nothing passed in is
        changed.  Returns a dict: state, trajectory, ntrajectory (afterwards), status (TRACK_FULL | TRACK_BAD_INDEX: nothing
        changed).  Raises ValueError for what pgorb_track_commit refuses."""
        fn = "Tracking.CommitFrame"
        P, Pp = Tracking._kf_poses(fn, kf_poses)
        traj = np.array(np.ascontiguousarray(trajectory, TRAJECTORY_RECORD_DTYPE).reshape(-1))
        if len(traj) > TRAJ_MAX_RECORDS or int(ntrajectory) < 0:
            raise ValueError(fn + ": more than TRAJ_MAX_RECORDS records, or a negative count")
        st = np.array(np.ascontiguousarray(state, TRACK_STATE_DTYPE).reshape(()))
        po = np.ascontiguousarray(pose, KF_POSE_DTYPE).reshape(())
        cnt = np.array([int(ntrajectory)], np.int32)
        status = ext._check(ext._L.pgorb_track_commit(
            ext._h, _p(st), _p(po), int(bool(ok)), int(ref_kf), float(frame_time), int(frame_id), len(P), _p(Pp),
            _p(traj if len(traj) else np.zeros(1, TRAJECTORY_RECORD_DTYPE)), len(traj), _p(cnt)))
        return dict(state=st, trajectory=traj, ntrajectory=int(cnt[0]), status=int(status))

    # ---- the decisions between the numeric steps (include/pgorb.h: csrc/track_decide.hip).  Everywhere: n [nframes] = the frames'
    # slot counts, frame [ntrack] (None = frame t) = each tracker's frame, per-tracker rows [ntrack][cap].  Nothing passed in is changed.
    @staticmethod
    def _td_rows(fn, n, frame, rows, npoints, lo=-1):
        """(n, frame or None, ntrack, nframes, cap, the rows as int32 [ntrack][cap]), checked as the single calls check them"""
        n = np.ascontiguousarray(n, np.int32).reshape(-1)
        rows = [np.ascontiguousarray(r, np.int32) for r in rows]
        if any(r.ndim != 2 or r.shape != rows[0].shape for r in rows):
            raise ValueError(fn + ": the slot arrays are [ntrack][cap_per_frame]")
        ntrack, cap = rows[0].shape
        fr = None if frame is None else _arr(frame, np.int32, ntrack, fn + " frame")
        if ntrack > TRACK_MAX or len(n) > COVIS_MAX_KF or cap > 16000:
            raise ValueError(fn + ": more than TRACK_MAX trackers, COVIS_MAX_KF frames or 16000 keypoints per frame")
        if len(n) and (n.min() < 0 or n.max() > cap):
            raise ValueError(fn + ": a frame's count is outside [0, cap_per_frame]")
        f = np.arange(ntrack, dtype=np.int32) if fr is None else fr
        if ntrack and (f.min() < 0 or f.max() >= len(n)):
            raise ValueError(fn + ": a tracker's frame is out of range")
        for r in rows:
            for t in range(ntrack):
                u = r[t, :n[f[t]]]
                if len(u) and (u.min() < lo or u.max() >= npoints):
                    raise ValueError(fn + ": a slot names a point out of range")
        return n, fr, ntrack, len(n), cap, rows

    @staticmethod
    def _td_obs(fn, npoints, obs_start, obs_frame, obs_live, nframes):
        st = _arr(obs_start, np.int32, npoints + 1, fn + " obs_start")
        of = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
        lv = None if obs_live is None else _arr(obs_live, np.uint8, len(of), fn + " obs_live")
        if st[0] != 0 or st[-1] != len(of) or np.any(np.diff(st) < 0):
            raise ValueError(fn + ": obs_start does not rise from 0 to nobs")
        live = of if lv is None else of[lv != 0]
        if len(live) and (live.min() < 0 or live.max() >= nframes):
            raise ValueError(fn + ": a live observation names a frame out of range")
        return st, (of if len(of) else np.zeros(1, np.int32)), lv, len(of)

    @staticmethod
    def _opt(a):
        return None if a is None else _p(a)

    @staticmethod
    def CheckReplacedInLastFrame(ext, last_point, n, npoints, replaced, frame=None):
        """Tracking::CheckReplacedInLastFrame (Tracking.cc:735-745) for every tracker: a slot p with replaced[p] >= 0 becomes
        replaced[p], ONE step.  Returns the slots afterwards.  Raises ValueError for what pgorb_check_replaced refuses."""
        fn = "Tracking.CheckReplacedInLastFrame"
        n, fr, ntrack, nframes, cap, (lp,) = Tracking._td_rows(fn, n, frame, [last_point], int(npoints))
        rp = _arr(replaced, np.int32, int(npoints), fn + " replaced")
        if len(rp) and (rp.min() < -1 or rp.max() >= npoints):
            raise ValueError(fn + ": a replacement is out of range")
        out = np.array(lp)
        ext._check(ext._L.pgorb_check_replaced(ext._h, ntrack, _p(n), nframes, cap, Tracking._opt(fr), _p(out), int(npoints), _p(rp)))
        return out

    @staticmethod
    def _td_queries(fn, ntrack, nq, queries, npoints, extra):
        nq = _arr(nq, np.int32, ntrack, fn + " nq")
        q = np.ascontiguousarray(queries, np.int32)
        if q.ndim != 2 or q.shape[0] != ntrack or q.shape[1] > 16000 or (extra is not None and np.shape(extra) != q.shape):
            raise ValueError(fn + ": the query arrays are [ntrack][qcap] with qcap <= 16000")
        if ntrack and (nq.min() < 0 or nq.max() > q.shape[1]):
            raise ValueError(fn + ": a query count is outside [0, qcap]")
        for t in range(ntrack):
            u = q[t, :nq[t]]
            if len(u) and (u.min() < 0 or u.max() >= npoints):
                raise ValueError(fn + ": a query names a point out of range")
        return nq, q

    @staticmethod
    def IncreaseVisible(ext, kp_point, n, nq, queries, in_view, visible, frame=None, run=None):
        """The two IncreaseVisible of SearchLocalPoints (Tracking.cc:1148, :1168) from SearchLocalPoints' kp_point_out and in_view.
        Returns visible afterwards."""
        fn = "Tracking.IncreaseVisible"
        vis = np.array(np.ascontiguousarray(visible, np.int32).reshape(-1))
        n, fr, ntrack, nframes, cap, (kp,) = Tracking._td_rows(fn, n, frame, [kp_point], len(vis))
        nq, q = Tracking._td_queries(fn, ntrack, nq, queries, len(vis), in_view)
        iv = np.ascontiguousarray(in_view, np.uint8)
        rn = None if run is None else _arr(run, np.uint8, ntrack, fn + " run")
        ext._check(ext._L.pgorb_increase_visible(ext._h, ntrack, _p(n), nframes, cap, Tracking._opt(fr), Tracking._opt(rn), _p(kp), q.shape[1],
                                                 _p(nq), _p(q), _p(iv), len(vis), _p(vis)))
        return vis

    @staticmethod
    def QuerySeenFromOutliers(ext, kp_point, outlier, n, nq, queries, npoints, frame=None, kp_point_opt=None):
        """The query_seen of SearchLocalPoints: the queries whose point sat in a slot that the first stage discarded (mnLastFrameSeen
        of Tracking.cc:781, :904).  kp_point = the slots BEFORE the discard; a slot was discarded when its outlier flag is set
        (outlier None = no flags) or when kp_point_opt, PoseOptimization's slots after a discard_outliers = True run (which clears
        the flags), differs from it.  Returns uint8 [ntrack][qcap], 0 past nq."""
        fn = "Tracking.QuerySeenFromOutliers"
        if npoints > 1048576:
            raise ValueError(fn + ": more than 1048576 points")
        if outlier is None and kp_point_opt is None:
            raise ValueError(fn + ": outlier or kp_point_opt is required")
        n, fr, ntrack, nframes, cap, rows = Tracking._td_rows(fn, n, frame, [kp_point] + ([] if kp_point_opt is None else [kp_point_opt]), int(npoints))
        kp, ko = rows[0], (rows[1] if len(rows) > 1 else None)
        ol = None if outlier is None else _arr(outlier, np.uint8, ntrack, fn + " outlier", cap)
        nq, q = Tracking._td_queries(fn, ntrack, nq, queries, int(npoints), None)
        seen = np.zeros(q.shape, np.uint8)
        ext._check(ext._L.pgorb_query_seen_from_outliers(ext._h, ntrack, _p(n), nframes, cap, Tracking._opt(fr), _p(kp), Tracking._opt(ol), Tracking._opt(ko), q.shape[1], _p(nq),
                                                         _p(q), int(npoints), _p(seen)))
        return seen

    @staticmethod
    def Decide(ext, mode, n, nmatches, nmatches_map, pose_before, kp_point_before, pose_opt, kp_point_opt, outlier, npoints, found, counters,
               point_has_obs=None, after_retry=False, frame=None, run=None):
        """bOK of one stage for every tracker and what the reference leaves in mCurrentFrame (include/pgorb.h: pgorb_track_decide).  mode =
        DECIDE_MOTION_MODEL | DECIDE_REFERENCE_KF | DECIDE_LOCAL_MAP, one for all or one per tracker.  Returns a dict: ok, inliers
        (LOCAL_MAP only, else 0), retry, pose_final, kp_point_final, found."""
        fn = "Tracking.Decide"
        n, fr, ntrack, nframes, cap, (kb, ko) = Tracking._td_rows(fn, n, frame, [kp_point_before, kp_point_opt], int(npoints))
        modes = None if np.ndim(mode) == 0 else _arr(mode, np.int32, ntrack, fn + " mode")
        if not set([int(mode)] if modes is None else modes.tolist()) <= {DECIDE_MOTION_MODEL, DECIDE_REFERENCE_KF, DECIDE_LOCAL_MAP}:
            raise ValueError(fn + ": an unknown mode")
        nm, mp = _arr(nmatches, np.int32, ntrack, fn + " nmatches"), _arr(nmatches_map, np.int32, ntrack, fn + " nmatches_map")
        pb, po = _arr(pose_before, KF_POSE_DTYPE, ntrack, fn + " pose_before"), _arr(pose_opt, KF_POSE_DTYPE, ntrack, fn + " pose_opt")
        ol = _arr(outlier, np.uint8, ntrack, fn + " outlier", cap)
        fd = np.array(_arr(found, np.int32, int(npoints), fn + " found"))
        ho = None if point_has_obs is None else _arr(point_has_obs, np.uint8, int(npoints), fn + " point_has_obs")
        ct = _arr(counters, TRACK_COUNTERS_DTYPE, ntrack, fn + " counters")
        rn = None if run is None else _arr(run, np.uint8, ntrack, fn + " run")
        ok, inl, rt = np.zeros(ntrack, np.uint8), np.zeros(ntrack, np.int32), np.zeros(ntrack, np.uint8)
        pf, kf = np.zeros(ntrack, KF_POSE_DTYPE), np.full((ntrack, cap), -1, np.int32)
        ext._check(ext._L.pgorb_track_decide(
            ext._h, ntrack, 0 if modes is not None else int(mode), Tracking._opt(modes), int(bool(after_retry)), _p(n), nframes, cap, Tracking._opt(fr),
            Tracking._opt(rn), _p(nm), _p(mp), _p(pb), _p(kb), _p(po), _p(ko), _p(ol), int(npoints), Tracking._opt(ho), _p(fd), _p(ct), _p(ok), _p(inl),
            _p(rt), _p(pf), _p(kf)))
        return dict(ok=ok, inliers=inl, retry=rt, pose_final=pf, kp_point_final=kf, found=fd)

    @staticmethod
    def FinishFrame(ext, n, ok, inliers, counters, pose_final, kp_point, outlier, npoints, obs_start, obs_frame, kf_point, kf_pose, kf_id,
                    point_bad=None, point_has_obs=None, obs_live=None, frame=None):
        """The tail of Tracking::Track for the trackers with ok (Tracking.cc:445-476): clean VO matches, NeedNewKeyFrame,
        CreateNewKeyFrame (the tracker's frame becomes the key frame), the outlier discard.  Returns a dict: counters, outlier,
        kf_point, kf_pose, kf_id (afterwards), kp_point_out (the next frame's last_point), ref_kf (what CommitFrame takes), new_kf,
        interrupt_ba, made."""
        fn = "Tracking.FinishFrame"
        n, fr, ntrack, nframes, cap, (kp,) = Tracking._td_rows(fn, n, frame, [kp_point], int(npoints))
        st, of, lv, nobs = Tracking._td_obs(fn, int(npoints), obs_start, obs_frame, obs_live, nframes)
        okk, inl = _arr(ok, np.uint8, ntrack, fn + " ok"), _arr(inliers, np.int32, ntrack, fn + " inliers")
        ct = np.array(_arr(counters, TRACK_COUNTERS_DTYPE, ntrack, fn + " counters"))
        pf = _arr(pose_final, KF_POSE_DTYPE, ntrack, fn + " pose_final")
        ol = np.array(_arr(outlier, np.uint8, ntrack, fn + " outlier", cap))
        kfp = np.array(_arr(kf_point, np.int32, nframes, fn + " kf_point", cap))
        kfq, kid = np.array(_arr(kf_pose, KF_POSE_DTYPE, nframes, fn + " kf_pose")), np.array(_arr(kf_id, np.uint64, nframes, fn + " kf_id"))
        pbad = None if point_bad is None else _arr(point_bad, np.uint8, int(npoints), fn + " point_bad")
        ho = None if point_has_obs is None else _arr(point_has_obs, np.uint8, int(npoints), fn + " point_has_obs")
        rows = (np.arange(ntrack) if fr is None else fr).tolist()
        if len(set(rows)) != ntrack:
            raise ValueError(fn + ": two trackers name one frame row")
        for t in range(ntrack):
            r = int(ct[t]["ref_kf"])
            if not 0 <= r < nframes or r in rows:
                raise ValueError(fn + ": a reference key frame is out of range or a tracker's frame row")
            u = kfp[r, :n[r]]
            if len(u) and (u.min() < -1 or u.max() >= npoints):
                raise ValueError(fn + ": a key frame's slot names a point out of range")
        out, ref, new, ib = np.full((ntrack, cap), -1, np.int32), np.zeros(ntrack, np.int32), np.zeros(ntrack, np.int32), np.zeros(ntrack, np.uint8)
        made = ext._check(ext._L.pgorb_track_finish(
            ext._h, ntrack, _p(n), nframes, cap, Tracking._opt(fr), _p(okk), _p(inl), _p(ct), _p(pf), _p(kp), _p(ol), int(npoints), Tracking._opt(pbad),
            Tracking._opt(ho), _p(st), _p(of), nobs, Tracking._opt(lv), _p(kfp), _p(kfq), _p(kid), _p(out), _p(ref), _p(new), _p(ib)))
        return dict(counters=ct, outlier=ol, kf_point=kfp, kf_pose=kfq, kf_id=kid, kp_point_out=out, ref_kf=ref, new_kf=new, interrupt_ba=ib,
                    made=int(made))

    @staticmethod
    def ScaleInitialMap(ext, kf_ini, kf_cur, kf_point, n, poses, points, obs_start, obs_frame, point_bad=None, obs_live=None):
        """CreateInitialMapMonocular's unit median depth (Tracking.cc:684-709).  Returns a dict: poses, points (afterwards), info
        [DECIDE_INFO] = (status, the median's float bits, TrackedMapPoints(1) of kf_cur, points scaled), median, wrong (the reference
        would reset: nothing was changed)."""
        fn = "Tracking.ScaleInitialMap"
        kfp, nn, P, X, npoints = LocalMapping._depth_table(fn, kf_point, n, poses, points)
        nframes, cap = kfp.shape
        if not (0 <= int(kf_ini) < nframes and 0 <= int(kf_cur) < nframes) or int(kf_ini) == int(kf_cur):
            raise ValueError(fn + ": a key frame is out of range, or both are one")
        st, of, lv, nobs = Tracking._td_obs(fn, npoints, obs_start, obs_frame, obs_live, nframes)
        pbad = None if point_bad is None else _arr(point_bad, np.uint8, npoints, fn + " point_bad")
        P, X, info = np.array(P), np.array(X if npoints else np.zeros(1, MAP_POINT_DTYPE)), np.zeros(DECIDE_INFO, np.int32)
        ext._check(ext._L.pgorb_scale_initial_map(ext._h, int(kf_ini), int(kf_cur), _p(kfp), _p(nn), nframes, cap, _p(P), npoints, _p(X),
                                                  Tracking._opt(pbad), _p(st), _p(of), nobs, Tracking._opt(lv), _p(info)))
        return dict(poses=P, points=X[:npoints], info=info, median=float(info[1:2].view(np.float32)[0]), wrong=bool(info[0] & DECIDE_WRONG_INIT))


# the trajectory read-out (include/pgorb.h): the records, the modes, the status bits and the limits
TRACK_STATE_DTYPE, TRAJECTORY_RECORD_DTYPE = _lib.TRACK_STATE_DTYPE, _lib.TRAJECTORY_RECORD_DTYPE
TRACK_MOTION_MODEL, TRACK_REFERENCE_KF = 0, 1
TRACK_NO_LAST, TRACK_NO_VELOCITY, TRACK_BAD_INDEX, TRACK_FULL, TRACK_MAX = 1, 2, 4, 8, 4096
TRAJ_BROKEN, TRAJ_BAD_TIME, TRAJ_NO_ORIGIN, TRAJ_INFO, TRAJ_MAX_RECORDS = 1, 2, 4, 4, 1 << 22
TCP_INFO = 4
# Tracking's decisions (include/pgorb.h): the counters record, the stages, the status bits and the limits
TRACK_COUNTERS_DTYPE = _lib.TRACK_COUNTERS_DTYPE
DECIDE_MOTION_MODEL, DECIDE_REFERENCE_KF, DECIDE_LOCAL_MAP, DECIDE_WRONG_INIT, DECIDE_INFO = 0, 1, 2, 4, 4
DEPTH_EMPTY, DEPTH_NAN, DEPTH_MAX_LIST = 1, 2, 262144


class System:
    """System::GetTrajectory (thirdparty/orb-slam2/src/System.cc:371-412) on the GPU, and the text form of its result that
    optical_trajectories --poses_in reads."""

    @staticmethod
    def GetTrajectory(ext, poses, kf_bad, parent, kf_id, tcp, trajectory):
        """poses / kf_bad / parent / kf_id (mnId) / tcp [nkf][12] (mTcp, read where kf_bad is set; None = zeros) = the key-frame
        table, trajectory = the TRAJECTORY_RECORD_DTYPE records of one tracker.  Returns a dict of the arrays
        pgorb_smooth_heading_directions / pgorb_trajectory_pca take as they are: quat_wxyz [n][4], translation [n][3] (float64),
        time_usec, frame_id (int64), is_lost (uint8), status (TRAJ_BROKEN per record), info [TRAJ_INFO], origin (key frame).
        Raises ValueError for everything pgorb_get_trajectory refuses."""
        fn = "System.GetTrajectory"
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        nkf = len(par)
        traj = np.ascontiguousarray(trajectory, TRAJECTORY_RECORD_DTYPE).reshape(-1)
        n = len(traj)
        if nkf > COVIS_MAX_KF or n > TRAJ_MAX_RECORDS:
            raise ValueError(fn + ": more than COVIS_MAX_KF key frames or TRAJ_MAX_RECORDS records")
        P = np.ascontiguousarray(poses, KF_POSE_DTYPE).reshape(-1)
        if len(P) != nkf:
            raise ValueError(fn + ": one pose per key frame")
        kb, ids = _arr(kf_bad, np.uint8, nkf, "kf_bad"), _arr(kf_id, np.uint64, nkf, "kf_id")
        tc = np.zeros((nkf, 12), np.float32) if tcp is None else _arr(tcp, np.float32, nkf, "tcp", 12)
        bad = kb != 0
        if not nkf or bad.all():
            raise ValueError(fn + ": no live key frame")
        if np.any((par[bad] < 0) | (par[bad] >= nkf)):
            raise ValueError(fn + ": a bad key frame has no parent or one out of range")
        t = traj["frame_time"]
        with np.errstate(over="ignore", invalid="ignore"):
            us = t * 1e6
        if not (np.isfinite(t).all() and np.all((us >= -2.0 ** 63) & (us < 2.0 ** 63))):
            raise ValueError(fn + ": a frame time is not finite or outside int64 microseconds")
        live = traj["lost"] == 0
        if np.any((traj["ref_kf"][live] < 0) | (traj["ref_kf"][live] >= nkf)):
            raise ValueError(fn + ": a record's reference key frame is out of range")
        n1 = max(n, 1)
        q, tr = np.zeros((n1, 4), np.float64), np.zeros((n1, 3), np.float64)
        tu, fi, lost, status, info = np.zeros(n1, np.int64), np.zeros(n1, np.int64), np.zeros(n1, np.uint8), np.zeros(n1, np.int32), \
            np.zeros(TRAJ_INFO, np.int32)
        ext._check(ext._L.pgorb_get_trajectory(ext._h, nkf, _p(P), _p(kb), _p(par), _p(ids), _p(tc), n,
                                               _p(traj if n else np.zeros(1, TRAJECTORY_RECORD_DTYPE)), _p(q), _p(tr), _p(tu), _p(fi), _p(lost),
                                               _p(status), _p(info)))
        return dict(quat_wxyz=q[:n], translation=tr[:n], time_usec=tu[:n], frame_id=fi[:n], is_lost=lost[:n], status=status[:n], info=info,
                    origin=int(info[1]))

    @staticmethod
    def write_poses(path, traj):
        """One `time_usec is_lost frame_id tx ty tz qw qx qy qz` line per record of a GetTrajectory result, the doubles with %.17g
        so that they round-trip: what optical_trajectories --poses_in=path reads."""
        with open(path, "w") as f:
            for i in range(len(traj["time_usec"])):
                v = list(traj["translation"][i]) + list(traj["quat_wxyz"][i])
                f.write("%d %d %d %s\n" % (int(traj["time_usec"][i]), int(traj["is_lost"][i]), int(traj["frame_id"][i]),
                                           " ".join("%.17g" % float(x) for x in v)))


# loop correction (include/pgorb.h): the status bits and the info lengths
LC_OVER_OBS, LC_BAD_INDEX, LC_INFO, MU_INFO = 1, 2, 4, 4


class LoopClosing:
    """The two map rewrites of loop closing (thirdparty/orb-slam2/src/LoopClosing.cc) on the GPU: CorrectLoop's propagation
    (:438-516) and the map update after global bundle adjustment (:679-742).  include/pgorb.h states both contracts."""

    @staticmethod
    def check_sim3(name, scw):
        S = np.ascontiguousarray(scw, SIM3D_DTYPE).reshape(1)
        if not (np.isfinite(S["r"]).all() and np.isfinite(S["t"]).all() and np.isfinite(S["s"]).all()):
            raise ValueError(name + ": scw is not finite")
        if not float(S["s"][0]) > 0.0:
            raise ValueError(name + ": the scale of scw is not positive")
        return S

    @staticmethod
    def check_poses(name, poses, nkf, what="poses"):
        P = np.ascontiguousarray(poses, KF_POSE_DTYPE).reshape(-1)
        if len(P) != nkf:
            raise ValueError("%s: %s needs one record per key frame" % (name, what))
        return P

    @staticmethod
    def CorrectLoopPoses(ext, octaves, poses, cur_kf, scw, connected, kf_point, points, obs_start, obs_frame, obs_idx, ref_obs, ref_kf,
                         point_bad=None, kf_order=None):
        """LoopClosing::CorrectLoop, :438-516 (without :515's UpdateConnections): the Sim3 correction of cur_kf's neighbourhood and
        of every map point it holds.  octaves[f] = mvKeysUn[i].octave of key frame f, poses KF_POSE_DTYPE, scw = mg2oScw
        (SIM3D_DTYPE), connected = mvpCurrentConnectedKFs by index (an entry that is negative, out of range or cur_kf is skipped;
        cur_kf is added), kf_point[f] the slots, the table as LocalMapping.RefreshMapPoints takes it, ref_kf[p] =
        GetReferenceKeyFrame() or -1, kf_order the address ranks (None = index order).  Nothing passed in is changed.  Returns a
        dict: has_corrected, corrected, has_non_corrected, non_corrected (what Optimizer.OptimizeEssentialGraph takes), poses,
        points, corrected_by, point_ref_kf, info [LC_INFO], status, members, corrected_points.  Raises ValueError for
        everything pgorb_correct_loop_poses refuses."""
        fn = "LoopClosing.CorrectLoopPoses"
        nkf = len(kf_point)
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))       # a copy: corrected in place
        n = len(pts)
        slots, ptrs, nk, st, of, pb, ko = _covis_table(fn, nkf, kf_point, n, obs_start, obs_frame, point_bad, kf_order)
        if not 0 <= int(cur_kf) < nkf:
            raise ValueError(fn + ": cur_kf is out of range")
        P = LoopClosing.check_poses(fn, poses, nkf)
        if not (np.isfinite(P["Tcw"]).all() and np.isfinite(P["Ow"]).all()):
            raise ValueError(fn + ": a pose is not finite")
        S = LoopClosing.check_sim3(fn, scw)
        if len(octaves) != nkf or any(len(o) != len(s) for o, s in zip(octaves, slots)):
            raise ValueError(fn + ": one octave per slot of every key frame")
        m = int(st[-1])
        oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
        if len(oi) < m or (m and (oi[:m].min() < 0 or np.any(oi[:m] >= nk[of[:m]]))):
            raise ValueError(fn + ": an observation names a keypoint out of range")
        if not np.isfinite(pts["pos"]).all():
            raise ValueError(fn + ": a point is not finite")
        ro, rk = _arr(ref_obs, np.int32, n, "ref_obs"), _arr(ref_kf, np.int32, n, "ref_kf")
        if n and (int(rk.min()) < -1 or int(rk.max()) >= nkf):
            raise ValueError(fn + ": ref_kf is out of range")
        ln = np.diff(st)
        if np.any((pb[:n] == 0) & (ln > 0) & (ln <= MP_MAX_OBS) & ((ro < 0) | (ro >= ln))):
            raise ValueError(fn + ": ref_obs lies outside the point's list")
        lst = np.ascontiguousarray(connected, np.int32).reshape(-1)
        if len(lst) > COVIS_MAX_KF:
            raise ValueError(fn + ": more than COVIS_MAX_KF list entries")
        keep = []
        kps = (C.c_void_p * max(nkf, 1))()
        for f, o in enumerate(octaves):
            k = np.zeros(max(len(o), 1), KEYPOINT_DTYPE)
            k["octave"][:len(o)] = o
            keep.append(k)
            kps[f] = k.ctypes.data
        one = np.zeros(1, np.int32)
        hc, hn = np.zeros(nkf, np.uint8), np.zeros(nkf, np.uint8)
        cor, non, po = np.zeros(nkf, SIM3D_DTYPE), np.zeros(nkf, SIM3D_DTYPE), np.zeros(nkf, KF_POSE_DTYPE)
        by, pr, info = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32), np.zeros(LC_INFO, np.int32)
        ret = ext._check(ext._L.pgorb_correct_loop_poses(
            ext._h, nkf, kps, _p(nk), _p(P), int(cur_kf), _p(S), len(lst), _p(lst if len(lst) else one), None if ko is None else _p(ko), ptrs, n,
            _p(pts if n else np.zeros(1, MAP_POINT_DTYPE)), _p(pb), _p(st), _p(of), _p(oi if len(oi) else one), _p(ro if n else one),
            _p(rk if n else one), _p(hc), _p(cor), _p(hn), _p(non), _p(po), _p(by), _p(pr), _p(info)))
        return dict(has_corrected=hc, corrected=cor, has_non_corrected=hn, non_corrected=non, poses=po, points=pts, corrected_by=by[:n].copy(),
                    point_ref_kf=pr[:n].copy(), info=info, status=int(info[0]), members=int(info[1]), corrected_points=int(ret))

    @staticmethod
    def CorrectLoopPoses_device(ext, d_kps, d_n, cap_per_frame, d_pose, cur_kf, d_scw, d_list, d_kf_point, npoints, d_points, d_obs_start,
                                d_obs_frame, d_obs_idx, d_ref_obs, d_ref_kf, d_point_bad=None, d_kf_order=None, d_list_count=None, stream=None):
        """pgorb_correct_loop_poses_device over resident torch tensors, asynchronous on `stream`: d_kps / d_pose / d_scw / d_points
        the bytes of their dtypes, the lists int32, the flags uint8; d_list may be a whole row of the covisibility graph's ord_kf
        with d_list_count = the one-element slice of nord (include/pgorb.h says why the count is needed).  The sizes and element
        types are checked here; the contents are not read.  d_points is corrected IN PLACE.  Returns a dict of freshly allocated
        tensors: has_corrected, corrected, has_non_corrected, non_corrected, pose_out (what Optimizer.OptimizeEssentialGraph_device
        takes), corrected_by, point_ref_kf and info [LC_INFO]."""
        import torch
        name = "LoopClosing.CorrectLoopPoses_device"
        for nm, t_ in (("d_n", d_n), ("d_list", d_list), ("d_kf_point", d_kf_point), ("d_obs_start", d_obs_start), ("d_obs_frame", d_obs_frame),
                       ("d_obs_idx", d_obs_idx), ("d_ref_obs", d_ref_obs), ("d_ref_kf", d_ref_kf), ("d_kf_order", d_kf_order),
                       ("d_list_count", d_list_count)):
            if t_ is not None and t_.dtype != torch.int32:
                raise ValueError("%s: %s must be an int32 tensor (the counts are taken from element counts)" % (name, nm))
        nkf, cap, npoints, nlist, nobs = int(d_n.numel()), int(cap_per_frame), int(npoints), int(d_list.numel()), int(d_obs_frame.numel())
        if not nkf or not 0 <= int(cur_kf) < nkf:
            raise ValueError(name + ": no key frame, or cur_kf is out of range")
        if cap < 1 or cap > 16000 or nkf > COVIS_MAX_KF or nlist > COVIS_MAX_KF or npoints < 0:
            raise ValueError(name + ": cap_per_frame outside [1, 16000], more than COVIS_MAX_KF key frames or list entries, or a negative count")
        if d_kps.numel() * d_kps.element_size() != nkf * cap * KEYPOINT_DTYPE.itemsize or int(d_kf_point.numel()) != nkf * cap or \
                d_pose.numel() * d_pose.element_size() != nkf * KF_POSE_DTYPE.itemsize or d_scw.numel() * d_scw.element_size() != SIM3D_DTYPE.itemsize:
            raise ValueError(name + ": d_kps and d_kf_point must be [nframes][cap], d_pose one record per frame, d_scw one record")
        if d_points.numel() * d_points.element_size() < npoints * MAP_POINT_DTYPE.itemsize or int(d_obs_start.numel()) != npoints + 1 or \
                int(d_obs_idx.numel()) != nobs or int(d_ref_obs.numel()) < npoints or int(d_ref_kf.numel()) < npoints:
            raise ValueError(name + ": the table, d_ref_obs or d_ref_kf is shorter than npoints, or d_obs_start is not npoints + 1")
        for nm, t_, need in (("d_point_bad", d_point_bad, npoints), ("d_kf_order", d_kf_order, nkf), ("d_list_count", d_list_count, 1)):
            if t_ is not None and t_.numel() < need:
                raise ValueError("%s: %s is too short" % (name, nm))
        dev = d_n.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(has_corrected=z((nkf,), torch.uint8), corrected=z((nkf, SIM3D_DTYPE.itemsize), torch.uint8),
                   has_non_corrected=z((nkf,), torch.uint8), non_corrected=z((nkf, SIM3D_DTYPE.itemsize), torch.uint8),
                   pose_out=z((nkf, KF_POSE_DTYPE.itemsize), torch.uint8), corrected_by=z((max(npoints, 1),), torch.int32),
                   point_ref_kf=z((max(npoints, 1),), torch.int32), info=z((LC_INFO,), torch.int32))
        q = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_correct_loop_poses_device(
            ext._h, q(d_kps), q(d_n), nkf, cap, q(d_pose), int(cur_kf), q(d_scw), nlist, q(d_list), q(d_list_count), q(d_kf_order), q(d_kf_point),
            npoints, q(d_points), q(d_point_bad), q(d_obs_start), q(d_obs_frame), q(d_obs_idx), nobs, q(d_ref_obs), q(d_ref_kf),
            q(out["has_corrected"]), q(out["corrected"]), q(out["has_non_corrected"]), q(out["non_corrected"]), q(out["pose_out"]),
            q(out["corrected_by"]), q(out["point_ref_kf"]), q(out["info"]), C.c_void_p(s)))
        return out

    @staticmethod
    def UpdateMapAfterGBA(ext, poses, poses_gba, kf_done, parent, kf_origin, points, pos_gba, point_done, ref_kf, kf_bad=None, point_bad=None):
        """LoopClosing::RunGlobalBundleAdjustment, :679-742: the spanning-tree propagation of the adjusted poses and the map points'
        update.  poses = the poses as they stand (mTcwBefGBA), poses_gba / kf_done / pos_gba / point_done as
        Optimizer.GlobalBundleAdjustment returns them, parent[f] or -1, kf_origin[f] = is in mvpKeyFrameOrigins, ref_kf[p] =
        GetReferenceKeyFrame() or -1.  Nothing passed in is changed.  Returns a dict: poses, kf_updated, points, point_updated, info
        [MU_INFO], updated (key frames), recomputed, updated_points.  Raises ValueError for everything pgorb_global_ba_map_update
        refuses."""
        fn = "LoopClosing.UpdateMapAfterGBA"
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        nkf = len(par)
        if nkf > COVIS_MAX_KF:
            raise ValueError(fn + ": more than COVIS_MAX_KF key frames")
        P, G = LoopClosing.check_poses(fn, poses, nkf), LoopClosing.check_poses(fn, poses_gba, nkf, "poses_gba")
        kd, ko, kb = _arr(kf_done, np.uint8, nkf, "kf_done"), _arr(kf_origin, np.uint8, nkf, "kf_origin"), _mask(kf_bad, nkf, "kf_bad")
        if nkf and (int(par.min()) < -1 or int(par.max()) >= nkf):
            raise ValueError(fn + ": a parent is out of range")
        u = kd != 0
        if not (np.isfinite(P["Tcw"]).all() and np.isfinite(P["Ow"]).all() and np.isfinite(G["Tcw"][u]).all() and np.isfinite(G["Ow"][u]).all()):
            raise ValueError(fn + ": a pose is not finite")
        mark = np.full(nkf, -1, np.int64)
        for k in range(nkf):
            cur = k
            while cur >= 0 and mark[cur] < 0:
                mark[cur] = k
                cur = int(par[cur])
            if cur >= 0 and mark[cur] == k:
                raise ValueError(fn + ": the parents form a cycle")
        pts = np.array(np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1))       # a copy: moved in place
        n = len(pts)
        pg, pd, pb = _arr(pos_gba, np.float32, n, "pos_gba", 3), _arr(point_done, np.uint8, n, "point_done"), _mask(point_bad, n, "point_bad")
        rk = _arr(ref_kf, np.int32, n, "ref_kf")
        if n and (int(rk.min()) < -1 or int(rk.max()) >= nkf):
            raise ValueError(fn + ": ref_kf is out of range")
        if not (np.isfinite(pts["pos"]).all() and np.isfinite(pg[pd != 0]).all()):
            raise ValueError(fn + ": a point is not finite")
        k1, n1 = max(nkf, 1), max(n, 1)
        po, ku, pu, info = np.zeros(k1, KF_POSE_DTYPE), np.zeros(k1, np.uint8), np.zeros(n1, np.uint8), np.zeros(MU_INFO, np.int32)
        pad = lambda x, dt, w=None: x if len(x) else np.zeros(1 if w is None else (1, w), dt)
        ret = ext._check(ext._L.pgorb_global_ba_map_update(
            ext._h, nkf, _p(pad(P, KF_POSE_DTYPE)), _p(pad(G, KF_POSE_DTYPE)), _p(pad(kd, np.uint8)), _p(pad(par, np.int32)), _p(pad(ko, np.uint8)),
            _p(kb), n, _p(pad(pts, MAP_POINT_DTYPE)), _p(pad(pg, np.float32, 3)), _p(pad(pd, np.uint8)), _p(pb), _p(pad(rk, np.int32)), _p(po), _p(ku),
            _p(pu), _p(info)))
        return dict(poses=po[:nkf].copy(), kf_updated=ku[:nkf].copy(), points=pts, point_updated=pu[:n].copy(), info=info, updated=int(ret),
                    recomputed=int(info[2]), updated_points=int(info[3]))

    @staticmethod
    def UpdateMapAfterGBA_device(ext, d_pose, d_pose_gba, d_kf_done, d_parent, d_kf_origin, npoints, d_points, d_pos_gba, d_point_done, d_ref_kf,
                                 d_kf_bad=None, d_point_bad=None, stream=None):
        """pgorb_global_ba_map_update_device over resident torch tensors, asynchronous on `stream`: d_pose / d_pose_gba / d_points the
        bytes of their dtypes, d_parent / d_ref_kf int32, d_pos_gba float32 [npoints][3], the flags uint8.  The sizes and element
        types are checked here; the contents are not read.  d_points[].pos is updated IN PLACE.  Returns a dict of freshly
        allocated tensors: pose_out, kf_updated, point_updated, info [MU_INFO]."""
        import torch
        name = "LoopClosing.UpdateMapAfterGBA_device"
        if d_parent.dtype != torch.int32 or d_ref_kf.dtype != torch.int32 or d_pos_gba.dtype != torch.float32:
            raise ValueError(name + ": d_parent and d_ref_kf must be int32 tensors, d_pos_gba float32")
        nkf, npoints = int(d_parent.numel()), int(npoints)
        if not nkf or nkf > COVIS_MAX_KF or npoints < 0:
            raise ValueError(name + ": no key frame, more than COVIS_MAX_KF, or a negative count")
        if d_pose.numel() * d_pose.element_size() != nkf * KF_POSE_DTYPE.itemsize or \
                d_pose_gba.numel() * d_pose_gba.element_size() != nkf * KF_POSE_DTYPE.itemsize or \
                d_kf_done.numel() * d_kf_done.element_size() != nkf or d_kf_origin.numel() * d_kf_origin.element_size() != nkf:
            raise ValueError(name + ": d_pose and d_pose_gba need one record, d_kf_done and d_kf_origin one byte per key frame")
        if d_points.numel() * d_points.element_size() < npoints * MAP_POINT_DTYPE.itemsize or int(d_pos_gba.numel()) < 3 * npoints or \
                d_point_done.numel() * d_point_done.element_size() < npoints or int(d_ref_kf.numel()) < npoints:
            raise ValueError(name + ": the table, d_pos_gba, d_point_done or d_ref_kf is shorter than npoints")
        for nm, t_, need in (("d_kf_bad", d_kf_bad, nkf), ("d_point_bad", d_point_bad, npoints)):
            if t_ is not None and t_.numel() * t_.element_size() < need:
                raise ValueError("%s: %s is too short" % (name, nm))
        dev = d_parent.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        out = dict(pose_out=z((nkf, KF_POSE_DTYPE.itemsize), torch.uint8), kf_updated=z((nkf,), torch.uint8),
                   point_updated=z((max(npoints, 1),), torch.uint8), info=z((MU_INFO,), torch.int32))
        q = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ext._check(ext._L.pgorb_global_ba_map_update_device(
            ext._h, nkf, q(d_pose), q(d_pose_gba), q(d_kf_done), q(d_parent), q(d_kf_origin), q(d_kf_bad), npoints, q(d_points), q(d_pos_gba),
            q(d_point_done), q(d_point_bad), q(d_ref_kf), q(out["pose_out"]), q(out["kf_updated"]), q(out["point_updated"]), q(out["info"]),
            C.c_void_p(s)))
        return out


class FrameStream:
    """Streamed ingest (include/pgorb.h, pgorb_stream_*): the frame loop around the extractor for frames that
    start in host memory -- ImageSequenceSource::next() -> System::TrackMonocular in the reference
    (src/slam/track_image_sequence.cc:43-47).  `depth` page-locked input slots of `batch` frames; submit() never
    blocks, wait() returns the batch's results as numpy views of page-locked memory."""

    def __init__(self, extractor, w, h, batch, depth=3, channels=1, rgb_order=True, rotate_degrees=0,
                 vertical_flip=False, horizontal_flip=False):
        """w x h: the frames AS DECODED (before rotation); channels 1 (grey), 3 (RGB24 / BGR24) or 4.  With anything but
        upright grey the slots hold the decoder's frames and rotation / flips / cvtColor run on the device in front of
        the pyramid (pgorb_stream_create_ingest; image_sequence_reader.cc:53-58,186-205, Tracking.cc:247-260)."""
        self.ext, self.w, self.h, self.batch, self.depth = extractor, int(w), int(h), int(batch), int(depth)
        self.channels = int(channels)
        self._L = extractor._L
        hs = C.c_void_p()
        extractor._check(self._L.pgorb_stream_create_ingest(extractor._h, self.w, self.h, self.channels, int(bool(rgb_order)),
                                                            int(rotate_degrees), int(bool(vertical_flip)), int(bool(horizontal_flip)),
                                                            self.batch, self.depth, C.byref(hs)))
        self._s = hs
        extractor._streams.add(self)

    def close(self):
        """Frees the page-locked slots: every array input() / wait() / frontend_results() returned is invalid afterwards."""
        if getattr(self, "_s", None):
            self._L.pgorb_stream_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _view(self, address, dtype, shape):
        """numpy view of page-locked memory the C stream owns.  The view keeps THIS object alive (its ctypes base holds a
        reference), so the memory is not freed by garbage collection while a result array is still in use; an explicit
        close() -- or submitting the slot again -- still invalidates it."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        buf = (C.c_uint8 * nbytes).from_address(address)
        buf._pgorb_owner = self
        return np.frombuffer(buf, dtype).reshape(shape)

    def input(self, slot):
        """numpy view [batch, h, w] (grey) or [batch, h, w, channels] of the slot's page-locked input frames: the decoder
        writes its frames here."""
        p = self._L.pgorb_stream_input(self._s, slot)
        shape = (self.batch, self.h, self.w) if self.channels == 1 else (self.batch, self.h, self.w, self.channels)
        return self._view(p, np.uint8, shape)

    def reset(self):
        self.ext._check(self._L.pgorb_stream_reset(self._s))

    def frontend(self, bounds, window_size=100, nnratio=0.9, check_orientation=True, bow_levelsup=-1):
        """Enable the per-frame front-end stage: grid, SearchForInitialization(previous, current) and -- with
        bow_levelsup >= 0 and a vocabulary uploaded to the extractor -- the BoW transform, on the device per batch."""
        self.ext._check(self._L.pgorb_stream_frontend(self._s, *[float(b) for b in bounds], int(window_size), float(nnratio),
                                                      int(bool(check_orientation)), int(bow_levelsup)))
        self._fe_bow = bow_levelsup >= 0

    def frontend_results(self, slot, nframes, cap):
        """(matches12[frames, cap], nmatches[frames], word, weight, node [frames, cap] or None) of a collected slot."""
        ptr = [C.c_void_p() for _ in range(5)]
        self.ext._check(self._L.pgorb_stream_frontend_results(self._s, slot, *[C.byref(p) for p in ptr]))

        def view(p, dtype, shape):
            return self._view(p.value, dtype, shape) if p.value else None
        return (view(ptr[0], np.int32, (nframes, cap)), view(ptr[1], np.int32, (nframes,)), view(ptr[2], np.uint32, (nframes, cap)),
                view(ptr[3], np.float64, (nframes, cap)), view(ptr[4], np.uint32, (nframes, cap)))

    def submit(self, slot, nframes=None):
        self.ext._check(self._L.pgorb_stream_submit(self._s, slot, self.batch if nframes is None else int(nframes)))

    def wait(self, slot):
        """(n[frames], kps[frames, cap], desc[frames, cap, 32], best_idx, best, second [frames, cap]) views."""
        ptr = [C.c_void_p() for _ in range(6)]
        cap = C.c_int32()
        nf = self.ext._check(self._L.pgorb_stream_wait(self._s, slot, *[C.byref(p) for p in ptr], C.byref(cap)))
        cap = cap.value

        def view(p, dtype, shape):
            return self._view(p.value, dtype, shape)
        return (view(ptr[0], np.int32, (nf,)), view(ptr[1], KEYPOINT_DTYPE, (nf, cap)), view(ptr[2], np.uint8, (nf, cap, 32)),
                view(ptr[3], np.int32, (nf, cap)), view(ptr[4], np.uint16, (nf, cap)), view(ptr[5], np.uint16, (nf, cap)))


class DeviceFrameStream:
    """The device-resident form of the stream (include/pgorb.h, pgorb_stream_create_device): frames are torch CUDA(HIP)
    uint8 tensors [B, H, W], results stay on the device, and `lanes` batches are in flight INSIDE the library (slot k
    runs on lane k % lanes, each lane an independent extractor working set on its own HIP stream).  Results equal the
    one-batch-at-a-time calls, including the match of a batch's first frame against the previous batch's last."""

    def __init__(self, extractor, w, h, batch, depth=2, lanes=2):
        self.ext, self.w, self.h, self.batch, self.depth = extractor, int(w), int(h), int(batch), int(depth)
        self._L = extractor._L
        hs = C.c_void_p()
        extractor._check(self._L.pgorb_stream_create_device(extractor._h, self.w, self.h, self.batch, self.depth, int(lanes), C.byref(hs)))
        self._s = hs
        self._keep = [None] * self.depth              # the submitted frame tensors (level 0 may alias them)
        extractor._streams.add(self)

    def close(self):
        if getattr(self, "_s", None):
            self._L.pgorb_stream_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lanes(self):
        return self._L.pgorb_stream_lanes(self._s)

    def reset(self):
        self.ext._check(self._L.pgorb_stream_reset(self._s))

    def frontend(self, bounds, window_size=100, nnratio=0.9, check_orientation=True, bow_levelsup=-1):
        self.ext._check(self._L.pgorb_stream_frontend(self._s, *[float(b) for b in bounds], int(window_size), float(nnratio),
                                                      int(bool(check_orientation)), int(bow_levelsup)))

    def submit(self, slot, frames_u8, stream=None):
        """Queue one batch; returns at once.  `frames_u8` must be ready on `stream` (default: torch's current stream)."""
        import torch
        nb, h, w = frames_u8.shape
        s = stream if stream is not None else torch.cuda.current_stream(frames_u8.device).cuda_stream
        self.ext._check(self._L.pgorb_stream_submit_device(self._s, slot, C.c_void_p(frames_u8.data_ptr()), nb, frames_u8.stride(1),
                                                           frames_u8.stride(0), C.c_void_p(s)))
        self._keep[slot] = frames_u8

    def wait(self, slot, on_host=True, stream=None):
        """(n[frames], kps[frames, cap, 7] f32 view, desc[frames, cap, 32], best_idx, best, second [frames, cap]) as torch
        tensors that ALIAS the slot's device result block (valid until the slot is submitted again)."""
        import torch
        ptr = [C.c_void_p() for _ in range(6)]
        cap = C.c_int32()
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        nf = self.ext._check(self._L.pgorb_stream_wait_device(self._s, slot, int(bool(on_host)), C.c_void_p(s),
                                                              *[C.byref(p) for p in ptr], C.byref(cap)))
        cap = cap.value
        dev = torch.device("cuda", self.ext.device)

        def view(p, dtype, shape, itemsize):
            return _device_tensor(p.value, int(np.prod(shape)) * itemsize, dev).view(dtype).reshape(shape)
        return (view(ptr[0], torch.int32, (nf,), 4), view(ptr[1], torch.float32, (nf, cap, 7), 4), view(ptr[2], torch.uint8, (nf, cap, 32), 1),
                view(ptr[3], torch.int32, (nf, cap), 4), view(ptr[4], torch.int16, (nf, cap), 2), view(ptr[5], torch.int16, (nf, cap), 2))


def _device_tensor(address, nbytes, device):
    """A torch uint8 tensor over `nbytes` of device memory the library owns (no copy): through the CUDA array interface."""
    import torch

    class _Raw:
        pass
    r = _Raw()
    r.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(address), False), "version": 2}
    return torch.as_tensor(r, device=device)
