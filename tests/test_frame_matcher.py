"""Frame grid (a12) and ORBmatcher::SearchForInitialization (a10): oracle self-checks on CPU,
GPU parity against the oracle."""
import numpy as np
import pytest

from pilotguru_amd.synth import synth_ride


def _frames(oracle, w=640, h=480, nf=1500, n=2, seed=4, dx=7, dy=3):
    ride = synth_ride(seed, w, h, n, dx=dx, dy=dy)
    ora = oracle.OrbOracle(nf, 1.2, 8, 20, 7)
    return ride, [ora.extract(ride[i]) for i in range(n)]


def test_oracle_grid_and_area_query(oracle):
    ride, fr = _frames(oracle)
    kps, desc = fr[0]
    bounds = (0.0, 640.0, 0.0, 480.0)
    start, idx = oracle.frame_grid(kps, bounds)
    assert start[-1] == len(kps) and sorted(idx.tolist()) == list(range(len(kps)))
    for c in (0, 100, 1500, 3071):                              # insertion order inside a cell
        cell = idx[start[c]:start[c + 1]]
        assert np.all(np.diff(cell) > 0)
    col = np.floor((kps["x"] - 0.0) * np.float32(64 / 640.0) + 0.5).astype(int)      # round(), positive
    row = np.floor((kps["y"] - 0.0) * np.float32(48 / 480.0) + 0.5).astype(int)
    for i in (0, 5, len(kps) - 1):
        c = col[i] * 48 + row[i]
        assert i in idx[start[c]:start[c + 1]]
    # brute-force area query, level 0 only
    got = oracle.features_in_area(kps, (start, idx), bounds, 300.0, 200.0, 100.0, 0, 0)
    want = [i for i in range(len(kps)) if kps["octave"][i] == 0 and abs(kps["x"][i] - 300) < 100 and abs(kps["y"][i] - 200) < 100]
    assert sorted(got.tolist()) == want
    # an out-of-image query returns nothing
    assert len(oracle.features_in_area(kps, (start, idx), bounds, 5000.0, 200.0, 100.0, 0, 0)) == 0


def test_oracle_search_for_initialization_finds_the_shift(oracle):
    ride, fr = _frames(oracle)
    (k1, d1), (k2, d2) = fr
    prev = np.stack([k1["x"], k1["y"]], 1)
    nm, m12, prev2 = oracle.search_for_initialization(k1, d1, k2, d2, (0.0, 640.0, 0.0, 480.0), prev)
    assert nm == int((m12 >= 0).sum()) and nm > 100
    lvl0 = k1["octave"] == 0
    assert np.all(m12[~lvl0] == -1)                              # only level-0 keypoints are matched
    dxy = np.stack([k2["x"][m12[m12 >= 0]] - k1["x"][m12 >= 0], k2["y"][m12[m12 >= 0]] - k1["y"][m12 >= 0]], 1)
    assert np.median(dxy[:, 0]) == -7 and np.median(dxy[:, 1]) == -3   # frame 1 = scene shifted by (7,3)
    assert len(set(m12[m12 >= 0].tolist())) == nm                # one-to-one
    assert np.array_equal(prev2[m12 >= 0], np.stack([k2["x"], k2["y"]], 1)[m12[m12 >= 0]])


SFI_CPP_DRIVER = r"""
// pgorb::ORBmatcher::SearchForInitialization (pilotguru_amd/host/orb_extractor.hpp) with a NULL context on well-formed and
// mis-sized input: prints what came back, or the exception it threw
#include <cstdio>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
int main()
{
    for (int v = 0; v < 6; v++) {
        Frame F1, F2;
        F1.mvKeysUndistorted.resize(4); F1.mDescriptors.resize(4 * 32);
        F2.mvKeysUndistorted.resize(5); F2.mDescriptors.resize(5 * 32);
        F2.mnMaxX = 640; F2.mnMaxY = 480;
        std::vector<float> prev(8);
        std::vector<int32_t> m12;
        if (v == 1) F1.mDescriptors.resize(3 * 32);
        if (v == 2) F2.mDescriptors.resize(6 * 32);
        if (v == 3) prev.resize(6);
        if (v == 4) prev.resize(10);
        if (v == 5) prev.clear();
        try {
            std::printf("%d\n", ORBmatcher(nullptr).SearchForInitialization(F1, F2, prev, m12));
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    return 0;
}
"""


def test_cpp_mirror_search_for_initialization_checks_sizes(tmp_path):
    """pgorb::ORBmatcher::SearchForInitialization refuses descriptor buffers that are not N x 32 bytes and a vbPrevMatched
    that is not 2 * N1 floats (std::invalid_argument) before any pointer reaches the library; well-formed input reaches it
    (here a NULL context, so the library's PGORB_E_ARG comes back as std::runtime_error)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = os.path.join(str(tmp_path), "sfi_driver.cc"), os.path.join(str(tmp_path), "sfi_driver")
    open(src, "w").write(SFI_CPP_DRIVER)
    lib = os.path.join(root, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", root, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.splitlines()
    assert out == ["runtime_error"] + ["invalid_argument"] * 5, out


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,ori,win", [(0.9, True, 100), (0.7, False, 40), (0.9, True, 8)])
def test_gpu_grid_and_search_for_initialization(oracle, ratio, ori, win):
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 1500
    ride = synth_ride(4, w, h, 2, dx=7, dy=3)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    for F in (F1, F2):
        start, idx = oracle.frame_grid(F.mvKeys, F.bounds)
        assert np.array_equal(F.grid_start, start) and np.array_equal(F.grid_idx[:len(idx)], idx)
    prev = np.stack([F1.mvKeys["x"], F1.mvKeys["y"]], 1).astype(np.float32)
    onm, om12, oprev = oracle.search_for_initialization(F1.mvKeys, F1.mDescriptors, F2.mvKeys, F2.mDescriptors,
                                                        F2.bounds, prev, win, ratio, ori)
    m = pg.ORBmatcher(ratio, ori)
    nm, m12 = m.SearchForInitialization(F1, F2, prev, win)
    assert nm == onm and np.array_equal(m12, om12)
    assert prev.tobytes() == oprev.tobytes()
    # second call with the updated vbPrevMatched (what MonocularInitialization does frame after frame)
    onm2, om12b, oprev2 = oracle.search_for_initialization(F1.mvKeys, F1.mDescriptors, F2.mvKeys, F2.mDescriptors,
                                                           F2.bounds, oprev, win, ratio, ori)
    nm2, m12b = m.SearchForInitialization(F1, F2, prev, win)
    assert nm2 == onm2 and np.array_equal(m12b, om12b) and prev.tobytes() == oprev2.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nf,nlev,win", [(480, 360, 3000, 2, 100), (400, 300, 2500, 1, 250), (640, 480, 1500, 8, 30)])
def test_gpu_search_for_initialization_dense_windows(oracle, w, h, nf, nlev, win):
    """Windows that hold more level-0 keypoints of F2 than the 64 candidates the parallel pass stores per F1 keypoint
    (k_sfi_candidates): those keypoints are evaluated in place by the sequential pass, in the reference's (column, row,
    insertion) order with the vMatchedDistance filter live (ORBmatcher.cc:440-457) -- mixed with stored lists in one
    frame pair.  The last case is the all-lists control."""
    import pilotguru_amd as pg
    ride = synth_ride(14, w, h, 2, dx=5, dy=2)
    ext = pg.ORBextractor(nf, 1.2, nlev, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    prev = np.stack([F1.mvKeys["x"], F1.mvKeys["y"]], 1).astype(np.float32)
    lvl0 = F2.mvKeys[F2.mvKeys["octave"] == 0]
    per_window = [int(((np.abs(lvl0["x"] - x) < win) & (np.abs(lvl0["y"] - y) < win)).sum()) for x, y in prev[F1.mvKeys["octave"] == 0][::7]]
    if win >= 100:
        assert max(per_window) > 64 and min(per_window) >= 1     # overflowed keypoints are present
    else:
        assert max(per_window) <= 64
    onm, om12, oprev = oracle.search_for_initialization(F1.mvKeys, F1.mDescriptors, F2.mvKeys, F2.mDescriptors, F2.bounds, prev, win, 0.9, True)
    nm, m12 = pg.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev, win)
    assert nm == onm and onm > 50 and np.array_equal(m12, om12) and prev.tobytes() == oprev.tobytes()


@pytest.mark.gpu
def test_gpu_search_for_initialization_batch_device(oracle):
    import ctypes as C
    import torch
    import pilotguru_amd as pg
    w, h, nf, B = 640, 480, 1000, 3
    ride = synth_ride(8, w, h, B, dx=5, dy=2)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    kps, desc, n = ext.extract_batch_device(torch.from_numpy(ride).cuda())
    cap = kps.shape[1]
    gs = torch.empty((B, 3073), dtype=torch.int32, device="cuda")
    gi = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(kps), p(n), B, cap, 0.0, float(w), 0.0, float(h), p(gs), p(gi), s))
    f1 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    f2 = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    prev = kps[:2, :, :2].contiguous().clone()
    m12 = torch.empty((2, cap), dtype=torch.int32, device="cuda")
    nm = torch.empty(2, dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_search_for_initialization_batch_device(
        ext._h, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(f1), p(f2), 2, 0.0, float(w), 0.0, float(h),
        p(prev), p(m12), p(nm), 100, 0.9, 1, s))
    torch.cuda.synchronize()
    nh = n.cpu().numpy()
    kh = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    dh = desc.cpu().numpy()
    for pi, (a, b) in enumerate(((0, 1), (1, 2))):
        ka = kh[a, :nh[a]].copy().view(oracle.KEYPOINT_DTYPE).reshape(-1)
        kb = kh[b, :nh[b]].copy().view(oracle.KEYPOINT_DTYPE).reshape(-1)
        pv = np.stack([ka["x"], ka["y"]], 1)
        onm, om12, oprev = oracle.search_for_initialization(ka, dh[a, :nh[a]], kb, dh[b, :nh[b]], (0.0, float(w), 0.0, float(h)), pv)
        assert int(nm[pi]) == onm
        assert np.array_equal(m12[pi, :nh[a]].cpu().numpy(), om12)
        assert prev[pi, :nh[a]].cpu().numpy().tobytes() == oprev.tobytes()


def _synthetic_map_points(F1keys, F1desc, shift, rng, drop=0.2, dup=0.1):
    """Map points 'seen' in frame 1, projected into frame 2 (= frame 1 shifted by `shift`), with
    jitter, a few invalid ones, a few without observations and duplicated descriptors (ties)."""
    n = len(F1keys)
    sel = rng.permutation(n)[: int(n * (1 - drop))]
    sel = np.concatenate([sel, sel[: int(n * dup)]])                       # duplicates compete for the same keypoint
    px = F1keys["x"][sel] - shift[0] + rng.uniform(-1.5, 1.5, len(sel)).astype(np.float32)
    py = F1keys["y"][sel] - shift[1] + rng.uniform(-1.5, 1.5, len(sel)).astype(np.float32)
    valid = (rng.uniform(size=len(sel)) > 0.05).astype(np.uint8)
    view_cos = np.where(rng.uniform(size=len(sel)) > 0.5, 0.9995, 0.9).astype(np.float32)
    has_obs = (rng.uniform(size=len(sel)) > 0.1).astype(np.uint8)
    return sel, valid, px.astype(np.float32), py.astype(np.float32), F1keys["octave"][sel].astype(np.int32), view_cos, F1desc[sel], has_obs


def test_oracle_search_by_projection_consistency(oracle):
    ride, fr = _frames(oracle, nf=1200)
    (k1, d1), (k2, d2) = fr
    rng = np.random.RandomState(3)
    sel, valid, px, py, lvl, vc, pd, obs = _synthetic_map_points(k1, d1, (7, 3), rng)
    sf = oracle.OrbOracle(1200).scale_factors
    bounds = (0.0, 640.0, 0.0, 480.0)
    nm, asg = oracle.search_by_projection_points(k2, d2, bounds, sf, None, valid, px, py, lvl, vc, pd, obs, 3.0, 0.8)
    assert nm > 300 and nm >= int((asg >= 0).sum())              # a point without observations can be overwritten
    good = asg >= 0
    assert np.all(valid[asg[good]] == 1)
    # assigned keypoints lie within the search radius of their point and in the allowed levels
    r = np.where(vc[asg[good]] > 0.998, 2.5, 4.0) * 3.0 * sf[lvl[asg[good]]]
    assert np.all(np.abs(k2["x"][good] - px[asg[good]]) < r) and np.all(np.abs(k2["y"][good] - py[asg[good]]) < r)
    assert np.all((k2["octave"][good] == lvl[asg[good]]) | (k2["octave"][good] == lvl[asg[good]] - 1))
    nm2, asg2 = oracle.search_by_projection_frame(k2, d2, bounds, sf, None, valid, px, py, lvl, k1["angle"][sel], pd, obs, 15.0)
    assert nm2 > 300 and nm2 <= int(valid.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("th,ratio", [(3.0, 0.8), (1.0, 0.8), (5.0, 0.6), (14.0, 0.6), (40.0, 0.9)])
def test_gpu_search_by_projection_points(oracle, th, ratio):
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 1200
    ride = synth_ride(4, w, h, 2, dx=7, dy=3)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    rng = np.random.RandomState(5)
    sel, valid, px, py, lvl, vc, pd, obs = _synthetic_map_points(F1.mvKeys, F1.mDescriptors, (7, 3), rng)
    has = (rng.uniform(size=F2.N) > 0.9).astype(np.uint8)         # some keypoints already hold a point
    onm, oasg = oracle.search_by_projection_points(F2.mvKeys, F2.mDescriptors, F2.bounds, ext.GetScaleFactors(), has,
                                                   valid, px, py, lvl, vc, pd, obs, th, ratio)
    nm, asg = pg.ORBmatcher(ratio, True).SearchByProjection(F2, pg.MapPoints(valid, px, py, lvl, vc, pd, obs), th, has)
    assert nm == onm and np.array_equal(asg, oasg) and nm > 100


@pytest.mark.gpu
@pytest.mark.parametrize("th,ori", [(15.0, True), (7.0, False), (30.0, True), (90.0, True)])
def test_gpu_search_by_projection_last_frame(oracle, th, ori):
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 1200
    ride = synth_ride(4, w, h, 2, dx=7, dy=3)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    rng = np.random.RandomState(6)
    sel, valid, px, py, lvl, vc, pd, obs = _synthetic_map_points(F1.mvKeys, F1.mDescriptors, (7, 3), rng)
    ang = F1.mvKeys["angle"][sel].copy()
    ang[::7] = (ang[::7] + 100.0) % 360.0                          # some rotation-inconsistent matches
    onm, oasg = oracle.search_by_projection_frame(F2.mvKeys, F2.mDescriptors, F2.bounds, ext.GetScaleFactors(), None,
                                                  valid, px, py, lvl, ang, pd, obs, th, ori)
    nm, asg = pg.ORBmatcher(0.9, ori).SearchByProjectionLastFrame(F2, valid, px, py, lvl, ang, pd, obs, th)
    assert nm == onm and np.array_equal(asg, oasg) and nm > 100


def _assert_lists_overflow(oracle, keys, bounds, windows, rows):
    """The premise of the pool-overflow test, from the oracle's GetFeaturesInArea alone: `windows` = (x, y, r, minLevel, maxLevel) of
    every query the reference evaluates against `keys`.  Some query has more survivors than the 64 fixed slots of its list, and the
    survivors beyond them, summed over the pair, exceed the pair's pool of rows * 256 entries.  (A query reserves pool space for an
    upper bound of its count, so the pool runs out no later than this sum says, and the queries behind are evaluated in place.)"""
    grid = oracle.frame_grid(keys, bounds)
    counts = np.array([len(oracle.features_in_area(keys, grid, bounds, *win)) for win in windows])
    assert counts.max() > 64
    assert int(np.maximum(counts - 64, 0).sum()) > rows * 256


@pytest.mark.gpu
def test_gpu_search_by_projection_when_the_list_pool_overflows(oracle):
    """One pyramid level, > 1 200 keypoints on 640 x 480 and search radii of 160 px: a query's window holds a third of the frame's
    keypoints, the lists of a pair add up to several times the pool (64 fixed + 256 pooled entries per query on average), and the
    later queries are marked LIST_OVER: they wait until every earlier query is decided and are evaluated in place.  All three forms."""
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 4000
    ride = synth_ride(14, w, h, 2, dx=5, dy=2)
    ext = pg.ORBextractor(nf, 1.2, 1, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    assert F2.N > 1200                                       # (radius 160 px: a window holds a third of them, > 64 + 256 per query)
    rng = np.random.RandomState(15)
    sf = ext.GetScaleFactors()
    sel, valid, px, py, lvl, vc, pd, obs = _synthetic_map_points(F1.mvKeys, F1.mDescriptors, (5, 2), rng)
    has = (rng.uniform(size=F2.N) > 0.9).astype(np.uint8)
    f32, live, osf = np.float32, np.flatnonzero(valid), oracle.OrbOracle(nf, 1.2, 1, 20, 7).scale_factors
    rvc = [f32(2.5) if float(vc[q]) > 0.998 else f32(4.0) for q in live]                     # RadiusByViewingCos (ORBmatcher.cc:133-139), then r*th, then * scale (:65-69)
    _assert_lists_overflow(oracle, F2.mvKeys, F2.bounds, [(px[q], py[q], f32(f32(r * f32(40.0)) * osf[lvl[q]]), int(lvl[q]) - 1, int(lvl[q]))
                                                          for q, r in zip(live, rvc)], len(valid))
    _assert_lists_overflow(oracle, F2.mvKeys, F2.bounds, [(px[q], py[q], f32(f32(160.0) * osf[lvl[q]]), int(lvl[q]) - 1, int(lvl[q]) + 1)
                                                          for q in live], len(valid))
    onm, oasg = oracle.search_by_projection_points(F2.mvKeys, F2.mDescriptors, F2.bounds, sf, has, valid, px, py, lvl, vc, pd, obs, 40.0, 0.7)
    nm, asg = pg.ORBmatcher(0.7, True).SearchByProjection(F2, pg.MapPoints(valid, px, py, lvl, vc, pd, obs), 40.0, has)
    assert nm == onm and np.array_equal(asg, oasg) and nm > 100
    ang = F1.mvKeys["angle"][sel].copy(); ang[::7] = (ang[::7] + 100.0) % 360.0
    onm, oasg = oracle.search_by_projection_frame(F2.mvKeys, F2.mDescriptors, F2.bounds, sf, None, valid, px, py, lvl, ang, pd, obs, 160.0, True)
    nm, asg = pg.ORBmatcher(0.9, True).SearchByProjectionLastFrame(F2, valid, px, py, lvl, ang, pd, obs, 160.0)
    assert nm == onm and np.array_equal(asg, oasg) and nm > 100
    # SearchForInitialization with a 250-px window on the same frames: lists beyond the fixed slots and, late in the pair, beyond the pool
    prev = np.stack([F1.mvKeys["x"], F1.mvKeys["y"]], 1).astype(np.float32)
    _assert_lists_overflow(oracle, F2.mvKeys, F2.bounds, [(x, y, f32(250), 0, 0) for (x, y), o in zip(prev, F1.mvKeys["octave"]) if o == 0],
                           max(F1.N, F2.N))
    onm, om12, oprev = oracle.search_for_initialization(F1.mvKeys, F1.mDescriptors, F2.mvKeys, F2.mDescriptors, F2.bounds, prev.copy(), 250, 0.9, True)
    nm, m12 = pg.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev, 250)
    assert nm == onm and np.array_equal(m12, om12) and prev.tobytes() == oprev.tobytes() and nm > 100


def _keyframe_queries(F1keys, F1desc, shift, rng, sf, nlevels, w, h):
    """Key-frame map points for the relocalisation search: projections near frame 2's keypoints (some outside the image
    bounds), depths whose predicted level is the keypoint's own level +- 1 (some outside the point's scale-invariance range),
    a few points already found."""
    sel, valid, px, py, lvl, _, pd, _ = _synthetic_map_points(F1keys, F1desc, shift, rng)
    nq = len(sel)
    px[::31] = -5.0; py[5::37] = np.float32(h + 3)                          # outside mnMinX / mnMaxY (:1512-1515)
    dist3d = rng.uniform(0.5, 30.0, nq).astype(np.float32)
    scale = np.float32(sf[1])
    # PredictScale = ceil(log(max / dist) / log(scale)): max = dist * scale^(level + d), d in (-1.5, 0.5) -> level - 1 .. level + 1
    maxd = (dist3d * scale ** (lvl.astype(np.float32) + rng.uniform(-1.5, 0.5, nq).astype(np.float32))).astype(np.float32)
    mind = (maxd / scale ** np.float32(nlevels - 1)).astype(np.float32)
    mind[3::41] = dist3d[3::41] * np.float32(1.5)                           # dist3D < 0.8f * mfMinDistance (:1525)
    maxd[7::43] = dist3d[7::43] * np.float32(0.5)                           # dist3D > 1.2f * mfMaxDistance
    found = (rng.uniform(size=nq) > 0.9).astype(np.uint8)
    ang = F1keys["angle"][sel].copy()
    ang[::7] = (ang[::7] + 100.0) % 360.0                                   # some rotation-inconsistent matches
    return sel, valid, found, px, py, dist3d, mind, maxd, ang, pd


def test_log_contract_and_predict_scale(oracle):
    """MapPoint::PredictScale (src/MapPoint.cc:516-531): `log` there is the platform's logf.  The contract (orc_log_f ==
    pgorb_log_f, a fixed double sequence rounded once) equals the correctly rounded logarithm on these samples, lies within
    1 ulp of this box's glibc logf, and the product's host code is the same function bit for bit."""
    import ctypes as C
    from pilotguru_amd import _lib
    L = _lib.lib()
    rng = np.random.RandomState(2)
    xs = np.concatenate([np.exp(rng.uniform(-30, 30, 20000)), rng.uniform(0.5, 2.0, 20000), np.float32(1.2) ** np.arange(-12, 13),
                         [1.0, 1e-45, 3.4e38, 2.0, 0.5, 1.4142135, 1.4142137]]).astype(np.float32)
    got = np.array([oracle.log_f(x) for x in xs], np.float32)
    exact = np.log(xs.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), exact.view(np.uint32))
    prod = np.array([L.pgorb_log_f(C.c_float(float(x))) for x in xs], np.float32)
    assert np.array_equal(prod.view(np.uint32), got.view(np.uint32))
    libm = C.CDLL("libm.so.6"); libm.logf.restype = C.c_float; libm.logf.argtypes = [C.c_float]
    glibc = np.array([libm.logf(float(x)) for x in xs], np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - glibc.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp > 0).mean() < 0.02
    assert oracle.log_f(0.0) == -np.inf and oracle.log_f(np.inf) == np.inf and np.isnan(oracle.log_f(np.nan))
    lf = oracle.log_f(np.float32(1.2))
    assert oracle.predict_scale(10.0, 10.0, lf, 8) == 0 and oracle.predict_scale(10.0, 20.0, lf, 8) == 0      # ratio <= 1 -> level 0
    assert oracle.predict_scale(12.5, 10.0, lf, 8) == 2                                                       # 1.25 > 1.2 -> ceil(1.22)
    assert oracle.predict_scale(1000.0, 1.0, lf, 8) == 7 and oracle.predict_scale(0.0, 1.0, lf, 8) == 0         # clamped; log(0) = -inf
    assert oracle.predict_scale(1.0, 0.0, lf, 8) == 0                     # ratio = inf: (int)ceil(inf) is INT_MIN on x86-64 -> 0


def test_predict_scale_under_the_log_contract_equals_glibc_at_the_level_boundaries(oracle):
    """`ceil(log(ratio) / mfLogScaleFactor)` (src/MapPoint.cc:524, Frame.cc:188) sits ON an integer whenever the
    ratio is a power of the scale factor, so a 1-ulp difference between the contract's log and the platform's logf could move
    a whole pyramid level.  Checked where it matters: ratios scaleFactor^k (the float products the reference's own tables
    hold, k = 0..8) and every float within 300 ulps of them, for six scale factors -- the level under the contract
    (orc_log_f == pgorb_log_f, bit-equal per the test above) equals the level glibc's logf gives in float arithmetic,
    32 454 ratios, no mismatch.  (Away from the boundaries a 1-ulp change of the logarithm cannot cross an integer.)"""
    import ctypes as C
    libm = C.CDLL("libm.so.6"); libm.logf.restype = C.c_float; libm.logf.argtypes = [C.c_float]
    total, mismatches = 0, []
    for sfv in (1.2, 1.1, 1.3, 1.5, 2.0, 1.05):
        sf = np.float32(sfv)
        lf_c, lf_g = oracle.log_f(sf), np.float32(libm.logf(float(sf)))
        assert np.float32(lf_c) == lf_g
        r = np.float32(1.0)
        for k in range(9):
            for d in range(-300, 301):
                x = (np.array([r]).view(np.int32) + d).view(np.float32)[0]
                got = oracle.predict_scale(float(x), 1.0, lf_c, 8)
                q = np.float32(np.float32(libm.logf(float(x))) / lf_g)
                want = min(max(int(np.ceil(q)), 0), 7)
                total += 1
                if got != want:
                    mismatches.append((sfv, k, d, got, want))
            r = np.float32(r * sf)
    assert total == 6 * 9 * 601 and mismatches == []


def test_oracle_search_by_projection_keyframe_consistency(oracle):
    ride, fr = _frames(oracle, nf=1200)
    (k1, d1), (k2, d2) = fr
    rng = np.random.RandomState(8)
    ora = oracle.OrbOracle(1200)
    sf = ora.scale_factors
    sel, valid, found, px, py, dist3d, mind, maxd, ang, pd = _keyframe_queries(k1, d1, (7, 3), rng, sf, 8, 640, 480)
    bounds = (0.0, 640.0, 0.0, 480.0)
    lf = oracle.log_f(sf[1])
    nm, asg = oracle.search_by_projection_keyframe(k2, d2, bounds, sf, None, valid, found, px, py, dist3d, mind, maxd, lf, ang, pd, 10.0, 100, True)
    assert nm == int((asg >= 0).sum()) > 200                    # every assignment blocks its keypoint: one point per keypoint
    good = asg >= 0
    q = asg[good]
    assert np.all(valid[q] == 1) and np.all(found[q] == 0) and len(set(q.tolist())) == nm
    # depth inside GetMin/MaxDistanceInvariance() = 0.8f * mfMinDistance .. 1.2f * mfMaxDistance (MapPoint.cc:390-400)
    assert np.all((px[q] >= 0) & (px[q] <= 640) & (py[q] >= 0) & (py[q] <= 480) & (dist3d[q] >= np.float32(0.8) * mind[q]) &
                  (dist3d[q] <= np.float32(1.2) * maxd[q]))
    lv = np.array([oracle.predict_scale(maxd[i], dist3d[i], lf, 8) for i in q])
    assert np.all(np.abs(k2["octave"][good] - lv) <= 1)
    assert np.all(np.abs(k2["x"][good] - px[q]) < 10.0 * sf[lv]) and np.all(np.abs(k2["y"][good] - py[q]) < 10.0 * sf[lv])
    nm2, _ = oracle.search_by_projection_keyframe(k2, d2, bounds, sf, None, valid, found, px, py, dist3d, mind, maxd, lf, ang, pd, 3.0, 64, True)
    assert 0 < nm2 <= nm
    # kp_has_point blocks: with every keypoint taken nothing is assigned
    nm3, asg3 = oracle.search_by_projection_keyframe(k2, d2, bounds, sf, np.ones(len(k2), np.uint8), valid, found, px, py, dist3d, mind, maxd, lf, ang, pd, 10.0, 100, True)
    assert nm3 == 0 and np.all(asg3 == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("th,orbdist,ori", [(10.0, 100, True), (3.0, 64, True), (10.0, 100, False), (6.0, 256, True), (70.0, 100, True)])
def test_gpu_search_by_projection_keyframe(oracle, th, orbdist, ori):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1476-1603) at the two
    call sites of Tracking::Relocalization (Tracking.cc:1434: 10 / 100; :1448: 3 / 64), without the orientation check, and
    with an ORBdist that accepts everything."""
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 1200
    ride = synth_ride(4, w, h, 2, dx=7, dy=3)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    rng = np.random.RandomState(9)
    sf = ext.GetScaleFactors()
    sel, valid, found, px, py, dist3d, mind, maxd, ang, pd = _keyframe_queries(F1.mvKeys, F1.mDescriptors, (7, 3), rng, sf, 8, w, h)
    lf = ext.log_scale_factor()
    assert np.float32(lf).view(np.uint32) == np.float32(oracle.log_f(sf[1])).view(np.uint32)
    for i in range(0, len(sel), 97):
        assert ext.predict_scale(maxd[i], dist3d[i]) == oracle.predict_scale(maxd[i], dist3d[i], lf, 8)
    has = (rng.uniform(size=F2.N) > 0.9).astype(np.uint8)
    onm, oasg = oracle.search_by_projection_keyframe(F2.mvKeys, F2.mDescriptors, F2.bounds, sf, has, valid, found, px, py, dist3d, mind, maxd,
                                                     lf, ang, pd, th, orbdist, ori)
    nm, asg = pg.ORBmatcher(0.9, ori).SearchByProjectionKeyFrame(F2, valid, found, px, py, dist3d, mind, maxd, ang, pd, th, orbdist, has)
    assert nm == onm and np.array_equal(asg, oasg) and nm > 50


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,ori", [(0.7, True), (0.9, False)])
def test_gpu_search_by_bow(tmp_path, oracle, ratio, ori):
    """TrackReferenceKeyFrame: ComputeBoW on both frames, then SearchByBoW(keyframe, frame)."""
    import os
    import pilotguru_amd as pg
    from pilotguru_amd import vocab as V
    w, h, nf = 640, 480, 1200
    ride = synth_ride(4, w, h, 2, dx=3, dy=1)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    KF, F = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
    desc, weight, parent = V.synth_vocabulary(6, 4, seed=4)
    path = os.path.join(str(tmp_path), "voc.txt")
    V.write_vocabulary_text(path, 6, 4, desc, weight, parent)
    voc = V.ORBVocabulary(text_file=path)
    voc.upload(ext)
    _, fvK = voc.transform(KF.mDescriptors, 2)                   # nodes 2 levels above the leaves
    _, fvF = voc.transform(F.mDescriptors, 2)
    rng = np.random.RandomState(8)
    valid = (rng.uniform(size=KF.N) > 0.3).astype(np.uint8)       # key-frame keypoints that carry a good map point
    onm, om = oracle.search_by_bow(KF.mDescriptors, KF.mvKeys["angle"], valid, fvK, F.mDescriptors, F.mvKeys["angle"], fvF, ratio, ori)
    nm, mt = pg.ORBmatcher(ratio, ori).SearchByBoW(ext, KF.mDescriptors, KF.mvKeys["angle"], valid, fvK, F, fvF)
    assert nm == onm and np.array_equal(mt, om) and nm > 50
    assert np.all(valid[mt[mt >= 0]] == 1) and len(set(mt[mt >= 0].tolist())) <= nm


def test_image_bounds_and_undistortion_oracle_properties(oracle):
    """cv::undistortPoints restatement: the fixed-point iteration inverts the distortion model."""
    from pilotguru_amd import _lib
    import ctypes as C
    cam, dist = (700.0, 690.0, 322.5, 238.25), (-0.25, 0.08, 0.001, -0.0007, 0.0)
    b = oracle.image_bounds(640, 480, cam, dist)
    assert b[0] < 0 and b[1] > 640 and b[2] < 0 and b[3] > 480       # barrel distortion: corners move outwards
    assert oracle.image_bounds(640, 480, cam, (0, 0, 0, 0, 0)) == (0.0, 640.0, 0.0, 480.0)
    got = np.zeros(4, np.float32)
    p = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    camf, df = np.array(cam, np.float32), np.array(dist, np.float32)
    assert _lib.lib().pgorb_image_bounds(640, 480, C.c_void_p(camf.ctypes.data), C.c_void_p(df.ctypes.data), C.c_void_p(got.ctypes.data)) == 0
    assert tuple(float(x) for x in got) == b                          # host function == oracle, bit for bit
    k = np.zeros(50, oracle.KEYPOINT_DTYPE)
    rng = np.random.RandomState(1)
    k["x"], k["y"] = rng.uniform(0, 640, 50), rng.uniform(0, 480, 50)
    u = oracle.undistort_keypoints(k, cam, dist)
    # forward model on the undistorted points reproduces the distorted ones
    x = (u["x"].astype(np.float64) - cam[2]) / cam[0]; y = (u["y"].astype(np.float64) - cam[3]) / cam[1]
    r2 = x * x + y * y
    cd = 1 + ((dist[4] * r2 + dist[1]) * r2 + dist[0]) * r2
    xd = x * cd + 2 * dist[2] * x * y + dist[3] * (r2 + 2 * x * x)
    yd = y * cd + dist[2] * (r2 + 2 * y * y) + 2 * dist[3] * x * y
    assert np.allclose(xd * cam[0] + cam[2], k["x"], atol=2e-2) and np.allclose(yd * cam[1] + cam[3], k["y"], atol=2e-2)


@pytest.mark.gpu
def test_gpu_undistort_and_distorted_frame_pipeline(oracle):
    """Frame constructor with a calibrated camera (k1 != 0): UndistortKeyPoints, ComputeImageBounds,
    AssignFeaturesToGrid on the undistorted keypoints, then SearchForInitialization."""
    import pilotguru_amd as pg
    w, h, nf = 640, 480, 1200
    cam, dist = (700.0, 690.0, 322.5, 238.25), (-0.25, 0.08, 0.001, -0.0007, 0.0)
    ride = synth_ride(4, w, h, 2, dx=7, dy=3)
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    F1, F2 = pg.Frame(ext, ride[0], cam, dist), pg.Frame(ext, ride[1], cam, dist)
    for F in (F1, F2):
        ou = oracle.undistort_keypoints(F.mvKeys, cam, dist)
        assert F.mvKeysUndistorted.tobytes() == ou.tobytes()
        assert F.bounds == oracle.image_bounds(w, h, cam, dist)
        start, idx = oracle.frame_grid(ou, F.bounds)
        assert np.array_equal(F.grid_start, start) and np.array_equal(F.grid_idx[:len(idx)], idx)
        assert start[-1] <= F.N                                   # PosInGrid may drop keypoints outside the bounds
    prev = np.stack([F1.mvKeysUndistorted["x"], F1.mvKeysUndistorted["y"]], 1).astype(np.float32)
    onm, om12, oprev = oracle.search_for_initialization(F1.mvKeysUndistorted, F1.mDescriptors, F2.mvKeysUndistorted,
                                                        F2.mDescriptors, F2.bounds, prev, 100, 0.9, True)
    nm, m12 = pg.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev, 100)
    assert nm == onm and np.array_equal(m12, om12) and prev.tobytes() == oprev.tobytes() and nm > 100


@pytest.mark.gpu
def test_gpu_batched_resident_forms_of_the_slam_state_matchers(tmp_path, oracle):
    """pgorb_search_by_projection_{points,frame}_batch_device, pgorb_feature_vectors_batch_device and
    pgorb_search_by_bow_batch_device: a ride extracted on the device, every frame matched against map points 'seen' in
    its predecessor (ORBmatcher.cc:46-131, :1355-1474) and BoW-matched against its predecessor as the key frame
    (:161-290), all pairs in ONE launch each -- assignment arrays and counts of every pair against the oracle."""
    import ctypes as C
    import os
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd import vocab as V
    w, h, nf, B = 640, 480, 1200, 6
    shift = (5, 2)
    ride = synth_ride(9, w, h, B, dx=shift[0], dy=shift[1])
    ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    L, hdl = ext._L, ext._h
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kps, desc, n = ext.extract_batch_device(torch.from_numpy(ride).cuda())
    ext.check_async()
    cap = kps.shape[1]
    nh = n.cpu().numpy()
    kh = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    dh = desc.cpu().numpy()
    K = [kh[f, :nh[f]].copy().view(oracle.KEYPOINT_DTYPE).reshape(-1) for f in range(B)]
    D = [dh[f, :nh[f]].copy() for f in range(B)]
    bounds = (0.0, float(w), 0.0, float(h))
    gs = torch.empty((B, 64 * 48 + 1), dtype=torch.int32, device="cuda"); gi = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_frame_grid_batch_device(hdl, p(kps), p(n), B, cap, *bounds, p(gs), p(gi), s))
    # pair j: queries built from frame j, matched against frame j + 1
    npairs = B - 1
    rng = np.random.RandomState(11)
    Q = [_synthetic_map_points(K[j], D[j], shift, rng) for j in range(npairs)]
    qcap = max(len(q[0]) for q in Q) + 3
    def pack(idx, dtype, width=None):
        a = np.zeros((npairs, qcap) + ((width,) if width else ()), dtype)
        for j, q in enumerate(Q):
            a[j, :len(q[idx])] = q[idx]
        return torch.from_numpy(a).cuda()
    valid, px, py, lvl, vc, pd, obs = pack(1, np.uint8), pack(2, np.float32), pack(3, np.float32), pack(4, np.int32), pack(5, np.float32), pack(6, np.uint8, 32), pack(7, np.uint8)
    ang_np = np.zeros((npairs, qcap), np.float32)
    for j, q in enumerate(Q):
        a = K[j]["angle"][q[0]].copy(); a[::7] = (a[::7] + 100.0) % 360.0
        ang_np[j, :len(a)] = a
    ang = torch.from_numpy(ang_np).cuda()
    nq = torch.tensor([len(q[0]) for q in Q], dtype=torch.int32, device="cuda")
    has_np = (rng.uniform(size=(npairs, cap)) > 0.9).astype(np.uint8)
    has = torch.from_numpy(has_np).cuda()
    pair_frame = torch.arange(1, B, dtype=torch.int32, device="cuda")
    asg = torch.empty((npairs, cap), dtype=torch.int32, device="cuda"); nm = torch.empty(npairs, dtype=torch.int32, device="cuda")
    sf = ext.GetScaleFactors()
    # (th 12 / 60: DENSE windows, most queries hold more than the 64 candidates of their fixed list slots -- the rest of a list lives
    #  in the pair's pool; rounds 2-3 re-evaluated such queries in place, the "initialisation workload cliff" of VERDICT r3)
    for th, ratio in ((3.0, 0.8), (1.0, 0.8), (12.0, 0.7)):
        ext._check(L.pgorb_search_by_projection_points_batch_device(hdl, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(pair_frame), npairs, *bounds,
                   p(has), qcap, p(nq), p(valid), p(px), p(py), p(lvl), p(vc), p(pd), p(obs), th, ratio, p(asg), p(nm), s))
        torch.cuda.synchronize()
        for j, q in enumerate(Q):
            onm, oasg = oracle.search_by_projection_points(K[j + 1], D[j + 1], bounds, sf, has_np[j, :nh[j + 1]], q[1], q[2], q[3], q[4], q[5], q[6], q[7], th, ratio)
            assert int(nm[j]) == onm > 100 and np.array_equal(asg[j, :nh[j + 1]].cpu().numpy(), oasg), "points pair %d" % j
            assert bool((asg[j, nh[j + 1]:] == -1).all())
    for th, ori in ((15.0, True), (7.0, False), (60.0, True)):
        ext._check(L.pgorb_search_by_projection_frame_batch_device(hdl, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(pair_frame), npairs, *bounds,
                   None, qcap, p(nq), p(valid), p(px), p(py), p(lvl), p(ang), p(pd), p(obs), th, int(ori), p(asg), p(nm), s))
        torch.cuda.synchronize()
        for j, q in enumerate(Q):
            onm, oasg = oracle.search_by_projection_frame(K[j + 1], D[j + 1], bounds, sf, None, q[1], q[2], q[3], q[4], ang_np[j, :len(q[0])], q[6], q[7], th, ori)
            assert int(nm[j]) == onm > 100 and np.array_equal(asg[j, :nh[j + 1]].cpu().numpy(), oasg), "frame pair %d" % j
    # the relocalisation search (key-frame form), all pairs in one launch
    KQ = [_keyframe_queries(K[j], D[j], shift, rng, sf, 8, w, h) for j in range(npairs)]
    qcap2 = max(len(q[0]) for q in KQ) + 5
    def pack2(idx, dtype, width=None):
        a = np.zeros((npairs, qcap2) + ((width,) if width else ()), dtype)
        for j, q in enumerate(KQ):
            a[j, :len(q[idx])] = q[idx]
        return torch.from_numpy(a).cuda()
    kv, kfnd, ku, kvv, kd3, kmin, kmax, kang, kpd = (pack2(1, np.uint8), pack2(2, np.uint8), pack2(3, np.float32), pack2(4, np.float32), pack2(5, np.float32),
                                                    pack2(6, np.float32), pack2(7, np.float32), pack2(8, np.float32), pack2(9, np.uint8, 32))
    nq2 = torch.tensor([len(q[0]) for q in KQ], dtype=torch.int32, device="cuda")
    lf = ext.log_scale_factor()
    for th, orbdist, ori in ((10.0, 100, True), (3.0, 64, True)):
        ext._check(L.pgorb_search_by_projection_keyframe_batch_device(hdl, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(pair_frame), npairs, *bounds,
                   p(has), qcap2, p(nq2), p(kv), p(kfnd), p(ku), p(kvv), p(kd3), p(kmin), p(kmax), p(kang), p(kpd), lf, th, orbdist, int(ori), p(asg), p(nm), s))
        torch.cuda.synchronize()
        for j, q in enumerate(KQ):
            onm, oasg = oracle.search_by_projection_keyframe(K[j + 1], D[j + 1], bounds, sf, has_np[j, :nh[j + 1]], q[1], q[2], q[3], q[4], q[5], q[6], q[7],
                                                             lf, q[8], q[9], th, orbdist, ori)
            assert int(nm[j]) == onm > 30 and np.array_equal(asg[j, :nh[j + 1]].cpu().numpy(), oasg), "key-frame pair %d" % j
    # BoW: transform on the device, FeatureVectors on the device, key frame j vs frame j + 1
    vdesc, weight, parent = V.synth_vocabulary(6, 4, seed=4)
    path = os.path.join(str(tmp_path), "voc.txt")
    V.write_vocabulary_text(path, 6, 4, vdesc, weight, parent)
    voc = V.ORBVocabulary(text_file=path)
    voc.upload(ext)
    word = torch.empty((B, cap), dtype=torch.int32, device="cuda"); wt = torch.empty((B, cap), dtype=torch.float64, device="cuda")
    node = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_bow_transform_device(hdl, p(desc), B * cap, 2, p(word), p(wt), p(node), s))
    fvn = torch.empty((B, cap), dtype=torch.int32, device="cuda"); fvs = torch.empty((B, cap + 1), dtype=torch.int32, device="cuda")
    fvf = torch.empty((B, cap), dtype=torch.int32, device="cuda"); nfv = torch.empty(B, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_feature_vectors_batch_device(hdl, p(node), p(n), B, cap, p(fvn), p(fvs), p(fvf), p(nfv), s))
    torch.cuda.synchronize()
    FV = []
    for f in range(B):
        _, fv = voc.transform(D[f], 2)                                   # host accumulation (pinned to the reference's FeatureVector.cpp)
        k = int(nfv[f])
        assert k == len(fv[0]) and np.array_equal(fvn[f, :k].cpu().numpy().astype(np.uint32), fv[0])
        assert np.array_equal(fvs[f, :k + 1].cpu().numpy(), fv[1]) and np.array_equal(fvf[f, :nh[f]].cpu().numpy().astype(np.uint32), fv[2])
        FV.append(fv)
    kfv_np = (rng.uniform(size=(npairs, cap)) > 0.3).astype(np.uint8)
    kfv = torch.from_numpy(kfv_np).cuda()
    pkf = torch.arange(0, B - 1, dtype=torch.int32, device="cuda")
    mt = torch.empty((npairs, cap), dtype=torch.int32, device="cuda")
    for ratio, ori in ((0.7, True), (0.9, False)):
        ext._check(L.pgorb_search_by_bow_batch_device(hdl, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfv), p(pkf), p(pair_frame), npairs,
                   p(kfv), ratio, int(ori), p(mt), p(nm), s))
        torch.cuda.synchronize()
        for j in range(npairs):
            onm, om = oracle.search_by_bow(D[j], K[j]["angle"], kfv_np[j, :nh[j]], FV[j], D[j + 1], K[j + 1]["angle"], FV[j + 1], ratio, ori)
            assert int(nm[j]) == onm > 50 and np.array_equal(mt[j, :nh[j + 1]].cpu().numpy(), om), "bow pair %d" % j
