"""ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:659-825, 142-159): the matcher of LocalMapping::CreateNewMapPoints.

CPU: the constructed cases of tests/triangulation_cases.py reach every edge in the plain reference
(tests/triangulation_reference.py), every wrong reading of a rule (triangulation_reference.MUTANTS) changes some case, and the
library exports the two entry points.  GPU: the single call and the batched device form equal the reference on every
constructed case and on synthetic rides (FeatureVectors from a synthetic vocabulary, F12 and the epipole from chosen poses)."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulation_cases as TC  # noqa: E402
import triangulation_reference as T  # noqa: E402
from matcher_cases import NLEVELS, SCALE, SF  # noqa: E402
from pilotguru_amd.synth import synth_ride  # noqa: E402

# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("family", list(TC.FAMILIES))
def test_constructed_family_reaches_its_edges(family):
    hits = collections.Counter()
    cases = [c for c in TC.all_cases(0) if c["family"] == family]
    assert cases
    for c in cases:
        TC.run_reference(c, hits=hits)
    missed = [t for t in TC.TARGETS[family] if hits[t] == 0]
    assert not missed, "family %s never reached %s (hits %s)" % (family, missed, dict(hits))


def test_constructed_cases_reach_matches_and_rejections():
    res = [TC.run_reference(c) for c in TC.all_cases(1)]
    assert any(r[0] > 0 for r in res) and any(r[0] == 0 for r in res)


def test_every_rule_mutant_is_caught():
    cases = TC.all_cases(2)
    want = [TC.run_reference(c) for c in cases]
    for name, rules in T.MUTANTS.items():
        caught = [c["name"] for c, w in zip(cases, want) if not TC.same(TC.run_reference(c, rules), w)]
        assert caught, "mutant %s agrees with the reference on every constructed case" % name


def test_constructed_expectations():
    """A few outcomes spelled out, so that the reference itself is pinned to the upstream text."""
    got = {c["name"]: TC.run_reference(c) for c in TC.all_cases(3)}
    assert got["dist 50 kept"][1].tolist() == [1] and got["dist 51 never kept"][0] == 0
    assert got["equal distances: the later passing one wins"][1].tolist() == [1]
    assert got["equal distances: the later one fails the line"][1].tolist() == [0]
    assert got["closer candidate fails the line, bestDist stays"][1].tolist() == [1]
    assert got["two KF1 keypoints share one KF2 keypoint"][1].tolist() == [0, 0]
    assert got["has_point1 skips"][1].tolist() == [-1, 0] and got["has_point2 skips the best"][1].tolist() == [1]
    assert got["subnormal den, num == 0"][0] == 1 and got["den == 0"][0] == 0
    assert got["node with 300 KF2 keypoints"][1].tolist() == [280, 100, -1]
    assert got["0.1 rule: 10 and 1 kept"][0] == 11 and got["0.1 rule: 11 and 1 dropped"][0] == 11
    assert T.matched_pairs(got["has_point1 skips"][1]) == [(1, 0)]


def test_search_for_triangulation_symbols_and_null_context():
    """The two entry points are exported and declared; a NULL context is PGORB_E_ARG (no device needed)."""
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in ("pgorb_search_for_triangulation", "pgorb_search_for_triangulation_batch_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    F = (C.c_float * 9)()
    assert L.pgorb_search_for_triangulation(None, None, None, None, 0, None, None, None, 0, None, None, None, 0, None, None, None, 0,
                                            F, 0.0, 0.0, 1, None) == _lib.PGORB_E_ARG
    assert L.pgorb_search_for_triangulation_batch_device(None, None, None, None, 1, None, None, None, None, None, None, 0, None, None,
                                                         None, None, 1, None, None, None) == _lib.PGORB_E_ARG
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgorb.h")).read()
    assert "int  pgorb_search_for_triangulation(" in header and "int  pgorb_search_for_triangulation_batch_device(" in header
    import pilotguru_amd as pg
    assert hasattr(pg.ORBmatcher, "SearchForTriangulation")


# ---------------------------------------------------------------- GPU
def _extractor(nf=1000, w=640, h=480, batch=1):
    import pilotguru_amd as pg
    ext = pg.ORBextractor(nf, SCALE, NLEVELS, 20, 7, max_width=w, max_height=h, max_batch=batch)
    assert np.array_equal(ext.GetScaleFactors(), SF) and np.array_equal(ext.GetScaleSigmaSquares(), TC.S2)
    return ext


@pytest.mark.gpu
def test_gpu_single_call_equals_reference_on_constructed_cases():
    ext = _extractor()
    bad = []
    for c in TC.all_cases(0):
        want, got = TC.run_reference(c), TC.run_gpu(c, ext)
        if not TC.same(want, got):
            bad.append("%s: reference %r, device %r" % (c["name"], want, got))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_gpu_single_call_argument_checks():
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    ext = _extractor()
    c = [c for c in TC.all_cases(0) if c["name"] == "dist 50 kept"][0]
    KF1, KF2 = TC.KeyFrameArrays(ext, c["k1"], c["d1"]), TC.KeyFrameArrays(ext, c["k2"], c["d2"])
    m = pg.ORBmatcher()
    nodes, start, feat = c["fv2"]
    with pytest.raises(_lib.PgorbError) as e:                       # a FeatureVector naming keypoint 2 of a 2-keypoint key frame
        m.SearchForTriangulation(KF1, KF2, c["F"], c["ep"], c["fv1"], (nodes, start, np.array([0, 2], np.uint32)))
    assert e.value.code == _lib.PGORB_E_ARG
    big = TC.KeyFrameArrays(ext, np.zeros(16001, KF1.mvKeys.dtype), np.zeros((16001, 32), np.uint8))
    with pytest.raises(_lib.PgorbError) as e:
        m.SearchForTriangulation(big, KF2, c["F"], c["ep"], c["fv1"], c["fv2"])
    assert e.value.code == _lib.PGORB_E_LIMIT


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_batched_form_equals_reference_on_constructed_cases(ori):
    ext = _extractor()
    cases = TC.all_cases(4)
    for c in cases:
        c["ori"] = ori
    res, mh, n1 = TC.run_gpu_batched(cases, ext)
    for j, (c, got) in enumerate(zip(cases, res)):
        assert TC.same(TC.run_reference(c), got), c["name"]
        assert (mh[j, n1[j]:] == -1).all(), c["name"]


def _vocabulary(tmp_path, ext):
    from pilotguru_amd import vocab as V
    desc, weight, parent = V.synth_vocabulary(6, 4, seed=4)
    path = os.path.join(str(tmp_path), "voc.txt")
    V.write_vocabulary_text(path, 6, 4, desc, weight, parent)
    voc = V.ORBVocabulary(text_file=path)
    voc.upload(ext)
    return voc


RIDE_SHIFT = (3, 1)


def _explain(m, K1, K2, F, ep, fv1, fv2, h1, h2, want, got):
    """What a disagreement looks like, for the failure message: the differing KF1 keypoints and whether the device repeats
    itself on the same inputs (a second call) -- so a failure can be told apart as wrong-but-stable or unstable."""
    again = m.SearchForTriangulation(K1, K2, F, ep, fv1, fv2, h1, h2)
    diff = np.flatnonzero(want[1] != got[1])
    return ("nmatches reference %d, device %d, repeated call %d (repeat %s the first call); %d KF1 keypoints differ, first %s"
            % (want[0], got[0], again[0], "equals" if TC.same(got, again) else "DIFFERS from", len(diff),
               [(int(i), int(want[1][i]), int(got[1][i])) for i in diff[:8]]))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,nf,levelsup", [(640, 480, 1200, 2), (1920, 1080, 2000, 3)])
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_synthetic_rides_equal_the_reference(tmp_path, oracle, w, h, nf, levelsup, ori):
    """Key frame 0 against key frames 1 and 2 of a ride (8 levels), random masks; a sideways pose along the ride's shift
    (far epipole) and a forward pose whose epipole sits on a matched KF2 keypoint.  levelsup 3 at 1080p puts 300-500 KF2
    keypoints in a node (the kernel's path outside the registers).  The matcher's inputs are pinned first (keypoints and
    descriptors equal the oracle's, FeatureVectors equal the oracle vocabulary's), so a disagreement is the matcher's."""
    import pilotguru_amd as pg
    ride = synth_ride(5, w, h, 3, dx=RIDE_SHIFT[0], dy=RIDE_SHIFT[1])
    ext = pg.ORBextractor(nf, SCALE, NLEVELS, 20, 7, max_width=w, max_height=h)
    KF = [pg.Frame(ext, ride[i]) for i in range(3)]
    ora = oracle.OrbOracle(nf, SCALE, NLEVELS, 20, 7)
    for i, K in enumerate(KF):
        ok, od = ora.extract(ride[i])
        assert K.mvKeys.tobytes() == ok.tobytes() and np.array_equal(K.mDescriptors, od), "extraction of frame %d differs from the oracle" % i
    voc = _vocabulary(tmp_path, ext)
    fv = [voc.transform(K.mDescriptors, levelsup)[1] for K in KF]
    ovoc = oracle.VocabOracle(os.path.join(str(tmp_path), "voc.txt"))
    for i, K in enumerate(KF):
        assert all(np.array_equal(x, y) for x, y in zip(fv[i], ovoc.transform(K.mDescriptors, levelsup)[1])), "FeatureVector %d" % i
    sf, s2 = ext.GetScaleFactors(), ext.GetScaleSigmaSquares()
    rng = np.random.RandomState(w)
    hits = collections.Counter()
    m = pg.ORBmatcher(0.6, ori)
    for a, b in ((0, 1), (0, 2)):
        K1, K2 = KF[a], KF[b]
        h1 = (rng.uniform(size=K1.N) < 0.3).astype(np.uint8)
        h2 = (rng.uniform(size=K2.N) < 0.3).astype(np.uint8)
        F, ep = TC.sideways_pose(b - a, RIDE_SHIFT, w, h)
        want = T.search_for_triangulation(K1.mvKeysUndistorted, K1.mDescriptors, h1, fv[a], K2.mvKeysUndistorted, K2.mDescriptors, h2,
                                          fv[b], F, ep, sf, s2, ori, hits=hits)
        got = m.SearchForTriangulation(K1, K2, F, ep, fv[a], fv[b], h1, h2)
        assert TC.same(want, got), "pair %r, sideways: %s" % ((a, b), _explain(m, K1, K2, F, ep, fv[a], fv[b], h1, h2, want, got))
        assert want[0] > 200, ((a, b), want[0])
        j = int(want[1][want[1] >= 0][0])
        F2, ep2 = TC.forward_pose((K2.mvKeysUndistorted["x"][j], K2.mvKeysUndistorted["y"][j]), w, h)
        want2 = T.search_for_triangulation(K1.mvKeysUndistorted, K1.mDescriptors, h1, fv[a], K2.mvKeysUndistorted, K2.mDescriptors, h2,
                                           fv[b], F2, ep2, sf, s2, ori, hits=hits)
        got2 = m.SearchForTriangulation(K1, K2, F2, ep2, fv[a], fv[b], h1, h2)
        assert TC.same(want2, got2), "pair %r, forward: %s" % ((a, b), _explain(m, K1, K2, F2, ep2, fv[a], fv[b], h1, h2, want2, got2))
        assert want2[0] > 100, ((a, b), want2[0])
    assert hits["epipole_rejected"] > 0 and hits["line_rejected"] > 0 and hits["kf1_has_point"] > 0 and hits["kf2_has_point"] > 0
    if levelsup == 3:
        assert hits["node_over_256"] > 0


@pytest.mark.gpu
def test_gpu_batched_form_on_a_ride_with_device_feature_vectors(tmp_path):
    """20-neighbour pair sets over a 32-frame ride plus an empty frame, FeatureVectors built on the device
    (pgorb_bow_transform_device -> pgorb_feature_vectors_batch_device), keypoint slots past n poisoned, a pair of a key frame with
    itself and pairs with the empty frame: every pair equals the reference and the single call."""
    import torch
    import pilotguru_amd as pg
    w, h, nf, B = 640, 480, 1000, 33
    ride = np.concatenate([synth_ride(6, w, h, 32, dx=RIDE_SHIFT[0], dy=RIDE_SHIFT[1]), np.zeros((1, h, w), np.uint8)])
    ext = pg.ORBextractor(nf, SCALE, NLEVELS, 20, 7, max_width=w, max_height=h, max_batch=B)
    L, hdl = ext._L, ext._h
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kps, desc, n = ext.extract_batch_device(torch.from_numpy(np.ascontiguousarray(ride)).cuda())
    ext.check_async()
    cap = kps.shape[1]
    nh = n.cpu().numpy()
    assert nh[32] == 0 and (nh[:32] > 500).all() and cap > nh.max()
    voc = _vocabulary(tmp_path, ext)
    word = torch.empty((B, cap), dtype=torch.int32, device="cuda"); wt = torch.empty((B, cap), dtype=torch.float64, device="cuda")
    node = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_bow_transform_device(hdl, p(desc), B * cap, 2, p(word), p(wt), p(node), s))
    fvn = torch.empty((B, cap), dtype=torch.int32, device="cuda"); fvs = torch.empty((B, cap + 1), dtype=torch.int32, device="cuda")
    fvf = torch.empty((B, cap), dtype=torch.int32, device="cuda"); nfv = torch.empty(B, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_feature_vectors_batch_device(hdl, p(node), p(n), B, cap, p(fvn), p(fvs), p(fvf), p(nfv), s))
    torch.cuda.synchronize()
    kh = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    K = [kh[f, :nh[f]].copy().view(TC.KEYPOINT_DTYPE).reshape(-1) for f in range(B)]
    D = [desc[f, :nh[f]].cpu().numpy() for f in range(B)]
    FV = []
    for f in range(B):
        k = int(nfv[f])
        FV.append((fvn[f, :k].cpu().numpy().astype(np.uint32), fvs[f, :k + 1].cpu().numpy(), fvf[f, :nh[f]].cpu().numpy().astype(np.uint32)))
    # poison every keypoint / descriptor slot past n (the kernels must not read them)
    kview = kps.view(torch.uint8).reshape(B, cap, 28)
    for f in range(B):
        kview[f, nh[f]:] = 0xFF
        desc[f, nh[f]:] = 0xAA
    # pairs: key frames 5 and 26 with 20 neighbours each, a key frame with itself, the empty frame on either side
    pairs = [(5, b) for b in range(32) if b != 5][:20] + [(26, b) for b in range(31, -1, -1) if b != 26][:20] + [(9, 9), (12, 32), (32, 12)]
    P = len(pairs)
    rng = np.random.RandomState(21)
    F = np.zeros((P, 9), np.float32); ep = np.zeros((P, 2), np.float32)
    for j, (a, b) in enumerate(pairs):
        if j % 2 == 0 or a == b:
            Fj, ej = TC.sideways_pose(max(abs(b - a), 1), RIDE_SHIFT, w, h)
        else:
            Fj, ej = TC.forward_pose((rng.uniform(50, w - 50), rng.uniform(50, h - 50)), w, h)
        F[j], ep[j] = Fj.reshape(9), ej
    h1 = (rng.uniform(size=(P, cap)) < 0.3).astype(np.uint8); h2 = (rng.uniform(size=(P, cap)) < 0.3).astype(np.uint8)
    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    pa, pb = T_(np.array([a for a, _ in pairs], np.int32)), T_(np.array([b for _, b in pairs], np.int32))
    m12 = torch.full((P, cap), -9, dtype=torch.int32, device="cuda"); nm = torch.full((P,), -9, dtype=torch.int32, device="cuda")
    dF, dE, dH1, dH2 = T_(F), T_(ep), T_(h1), T_(h2)                 # (held: the launch reads them after the call returns)
    sf, s2 = ext.GetScaleFactors(), ext.GetScaleSigmaSquares()
    total = 0
    for ori in (True, False):
        ext._check(L.pgorb_search_for_triangulation_batch_device(hdl, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfv), p(pa), p(pb), P,
                                                                p(dF), p(dE), p(dH1), p(dH2), int(ori), p(m12), p(nm), s))
        torch.cuda.synchronize()
        mh, nmh = m12.cpu().numpy(), nm.cpu().numpy()
        m = pg.ORBmatcher(0.6, ori)
        for j, (a, b) in enumerate(pairs):
            want = T.search_for_triangulation(K[a], D[a], h1[j, :nh[a]], FV[a], K[b], D[b], h2[j, :nh[b]], FV[b], F[j].reshape(3, 3), ep[j],
                                              sf, s2, ori)
            got = (int(nmh[j]), mh[j, :nh[a]].copy())
            assert TC.same(want, got), "pair %d %r ori %r" % (j, (a, b), ori)
            assert (mh[j, nh[a]:] == -1).all()
            one = m.SearchForTriangulation(TC.KeyFrameArrays(ext, K[a], D[a]), TC.KeyFrameArrays(ext, K[b], D[b]), F[j], ep[j], FV[a], FV[b],
                                           h1[j, :nh[a]], h2[j, :nh[b]])
            assert TC.same(one, got), "single call, pair %d" % j
            total += want[0]
        assert nmh[P - 2] == 0 and nmh[P - 1] == 0
    assert total > 20 * P
    # no mask at all (NULL): equals the reference with empty masks
    ext._check(L.pgorb_search_for_triangulation_batch_device(hdl, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfv), p(pa), p(pb), P,
                                                            p(dF), p(dE), None, None, 1, p(m12), p(nm), s))
    torch.cuda.synchronize()
    for j in (0, 1, 40):
        a, b = pairs[j]
        want = T.search_for_triangulation(K[a], D[a], None, FV[a], K[b], D[b], None, FV[b], F[j].reshape(3, 3), ep[j], sf, s2, True)
        assert TC.same(want, (int(nm[j]), m12[j, :nh[a]].cpu().numpy())), "no masks, pair %d" % j


# ---------------------------------------------------------------- the wrappers' own checks and the C++ mirror
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_wrapper_rejects_short_masks_and_inconsistent_feature_vectors():
    """The wrapper hands N mask entries, N descriptors and start[nfv] feature indices to the library by pointer: anything
    shorter is refused before a pointer is passed (no device needed, the checks come first)."""
    import pilotguru_amd as pg
    c = [c for c in TC.all_cases(0) if c["name"] == "has_point1 skips"][0]
    KF1, KF2 = TC.KeyFrameArrays(None, c["k1"], c["d1"]), TC.KeyFrameArrays(None, c["k2"], c["d2"])
    m = pg.ORBmatcher()
    bad = [dict(has_point1=c["h1"][:1]), dict(has_point2=np.zeros(3, np.uint8)),
           dict(fv1=(c["fv1"][0], c["fv1"][1][:1], c["fv1"][2])), dict(fv2=(c["fv2"][0], c["fv2"][1], c["fv2"][2][:0]))]
    for kw in bad:
        a = dict(fv1=c["fv1"], fv2=c["fv2"], has_point1=c["h1"], has_point2=c["h2"])
        a.update(kw)
        with pytest.raises(ValueError):
            m.SearchForTriangulation(KF1, KF2, c["F"], c["ep"], a["fv1"], a["fv2"], a["has_point1"], a["has_point2"])
    short = TC.KeyFrameArrays(None, c["k1"], c["d1"])
    short.mDescriptors = short.mDescriptors[:1]
    with pytest.raises(ValueError):
        m.SearchForTriangulation(short, KF2, c["F"], c["ep"], c["fv1"], c["fv2"])


CPP_DRIVER = r"""
// reads key-frame pairs written by tests/test_search_for_triangulation.py and prints what pgorb::ORBmatcher::SearchForTriangulation
// (pilotguru_amd/host/orb_extractor.hpp) returns: "nmatches i:j ..." or the exception it threw
#include <cstdio>
#include <cstring>
#include <fstream>
#include "pilotguru_amd/host/orb_extractor.hpp"
using namespace pgorb;
template <class T> static void rd(std::ifstream& f, std::vector<T>& v, int32_t n) { v.resize(n); if (n) f.read((char*)v.data(), (size_t)n * sizeof(T)); }
static int32_t i32(std::ifstream& f) { int32_t v; f.read((char*)&v, 4); return v; }
static void readKF(std::ifstream& f, Frame& K, FeatureVector& fv, std::vector<uint8_t>& has)
{
    const int32_t n = i32(f), nfv = i32(f), nstart = i32(f), nfeat = i32(f), nhas = i32(f);
    rd(f, K.mvKeysUndistorted, n); rd(f, K.mDescriptors, n * 32); rd(f, has, nhas);
    rd(f, fv.mNode, nfv); rd(f, fv.mStart, nstart); rd(f, fv.mFeat, nfeat);
}
int main(int argc, char** argv)
{
    const bool run = argc > 1 && std::strcmp(argv[1], "run") == 0;        // "check": no context, the wrapper's checks only
    ORBextractor* ext = run ? new ORBextractor(1000, 1.2f, 8, 20, 7, 640, 480) : nullptr;
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        const int32_t ori = i32(f);
        float F[9], ep[2];
        f.read((char*)F, sizeof F); f.read((char*)ep, sizeof ep);
        Frame K1, K2; FeatureVector fv1, fv2; std::vector<uint8_t> h1, h2;
        readKF(f, K1, fv1, h1); readKF(f, K2, fv2, h2);
        ORBmatcher m(ext ? ext->context() : nullptr, 0.6f, ori != 0);
        std::vector<std::pair<size_t, size_t> > pairs;
        try {
            const int n = m.SearchForTriangulation(K1, K2, fv1, fv2, F, ep[0], ep[1], h1, h2, pairs);
            std::printf("%d", n);
            for (size_t k = 0; k < pairs.size(); k++) std::printf(" %zu:%zu", pairs[k].first, pairs[k].second);
            std::printf("\n");
        } catch (const std::invalid_argument&) { std::printf("invalid_argument\n");
        } catch (const std::runtime_error&) { std::printf("runtime_error\n"); }
    }
    delete ext;
    return 0;
}
"""


def _cpp_driver(tmp_path):
    import subprocess
    src, exe = os.path.join(str(tmp_path), "tri_driver.cc"), os.path.join(str(tmp_path), "tri_driver")
    open(src, "w").write(CPP_DRIVER)
    lib = os.path.join(ROOT, "pilotguru_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", ROOT, src, "-o", exe, "-L", lib, "-lpgorb", "-Wl,-rpath," + lib,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _write_case(path, c, h1=None, h2=None, fv1=None, fv2=None):
    def kf(k, d, has, fv):
        fv = [np.asarray(x) for x in fv]
        head = np.array([len(k), len(fv[0]), len(fv[1]), len(fv[2]), len(has)], np.int32)
        return (head.tobytes() + np.ascontiguousarray(k).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes() +
                np.asarray(has, np.uint8).tobytes() + fv[0].astype(np.uint32).tobytes() + fv[1].astype(np.int32).tobytes() +
                fv[2].astype(np.uint32).tobytes())
    with open(path, "wb") as f:
        f.write(np.int32(c["ori"]).tobytes() + c["F"].astype(np.float32).tobytes() + np.array(c["ep"], np.float32).tobytes())
        f.write(kf(c["k1"], c["d1"], c["h1"] if h1 is None else h1, c["fv1"] if fv1 is None else fv1))
        f.write(kf(c["k2"], c["d2"], c["h2"] if h2 is None else h2, c["fv2"] if fv2 is None else fv2))


def _run_driver(exe, mode, paths):
    import subprocess
    out = subprocess.run([exe, mode] + paths, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    return out.splitlines()


def test_cpp_mirror_checks_sizes_before_calling_the_library(tmp_path):
    """pgorb::ORBmatcher::SearchForTriangulation refuses masks that are neither empty nor N long and FeatureVectors of
    inconsistent lengths (std::invalid_argument) before any pointer reaches the library; well-formed input reaches it (here a
    NULL context, so the library's PGORB_E_ARG comes back as std::runtime_error)."""
    exe = _cpp_driver(tmp_path)
    c = [c for c in TC.all_cases(0) if c["name"] == "has_point1 skips"][0]
    variants = [("well formed", {}), ("empty masks", dict(h1=np.zeros(0, np.uint8), h2=np.zeros(0, np.uint8))),
                ("short has_point1", dict(h1=c["h1"][:1])), ("long has_point2", dict(h2=np.zeros(3, np.uint8))),
                ("start of wrong length", dict(fv1=(c["fv1"][0], c["fv1"][1][:1], c["fv1"][2]))),
                ("features shorter than start[n]", dict(fv2=(c["fv2"][0], c["fv2"][1], c["fv2"][2][:0])))]
    paths = []
    for k, (_, kw) in enumerate(variants):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % k))
        _write_case(paths[-1], c, **kw)
    got = _run_driver(exe, "check", paths)
    assert got == ["runtime_error", "runtime_error"] + ["invalid_argument"] * 4, list(zip([v[0] for v in variants], got))


@pytest.mark.gpu
def test_gpu_cpp_mirror_equals_reference_on_constructed_cases(tmp_path):
    """The C++ mirror on a real context: vMatchedPairs and nmatches of every constructed case equal the reference's."""
    exe = _cpp_driver(tmp_path)
    cases = TC.all_cases(5)
    paths = []
    for k, c in enumerate(cases):
        paths.append(os.path.join(str(tmp_path), "case%d.bin" % k))
        _write_case(paths[-1], c)
    got = _run_driver(exe, "run", paths)
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        nm, m12 = TC.run_reference(c)
        want = " ".join(["%d" % nm] + ["%d:%d" % p for p in T.matched_pairs(m12)])
        assert line == want, "%s: reference %r, C++ mirror %r" % (c["name"], want, line)
