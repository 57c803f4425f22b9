"""Device time of the kernels either side of the hot path on the benchmark's batch:
128 frames of 1920x1080 / 2000 keypoints resident in HBM.  HIP events on the stream the calls are issued on, median of 9;
next to each, the oracle's CPU time for the same work (1 thread, a few frames, scaled to the batch).

  ingest       RGB -> grey (Tracking.cc:247-260) + horizontal flip (image_sequence_reader.cc:53-58) in front of K1
  undistort    Frame::UndistortKeyPoints (Frame.cc:408-438), k1 != 0
  grid         Frame::AssignFeaturesToGrid (Frame.cc:234-249), 64 x 48 cells, CSR
  init-match   ORBmatcher::SearchForInitialization (ORBmatcher.cc:407-522), window 100, every frame vs its predecessor
  bow          ORBVocabulary::transform (TemplatedVocabulary.h:1126-1259) on an ORBvoc-sized tree (k = 10, L = 6)
  triangulate  ORBmatcher::SearchForTriangulation (ORBmatcher.cc:659-825): one host pair, and key frames of the batch against
               20 neighbours each, as LocalMapping::CreateNewMapPoints calls it (LocalMapping.cc:212-270); no CPU column
  map points   LocalMapping::CreateNewMapPoints (LocalMapping.cc:209-454, monocular) for the same key frames and neighbours in one
               batched call, one key frame through the host API, and the 20 host matcher calls per key frame it replaces
  fuse         ORBmatcher::Fuse (ORBmatcher.cc:827-979) as SearchInNeighbors calls it: one call of 1500 points through the host API,
               and the same key frames x 20 targets as independent problems of the batched form; the CPU column is the Python
               reference's matching step (tests/fuse_reference.py) for one call
  refresh      MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (MapPoint.cc:259-388) of many points in one batched
               call: a key frame's tail (1500 points) and a local-BA-sized set (20000 points) of the skewed list-length
               distribution of tests/map_point_cases.py; beside it the download + host loop + upload it replaces, the host loop
               being OUR restatement (tests/map_point_reference.py, Python, one core), not ORB-SLAM2.  --refresh-only runs this row alone

  place        KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:212-310) as one batched resident call: 4096 key
               frames of about 1500 words, 64 queries; beside it a plain C++ std::map / std::list restatement of the same queries
               on one core (tools/place_comparator.py, compiled by the tool; OUR restatement, not ORB-SLAM2), whose results the
               GPU's must equal.  --place-only runs this row alone

  loop         loop closing's four matchers (ORBmatcher.cc:524-657, 1106-1330, 292-405, 981-1104) as batched resident calls on constructed
               scenes (tests/loop_cases.py): SearchByBoW(KF, KF) and SearchBySim3 on 8 pairs of about 2000 features,
               SearchByProjection(KF, Scw) with 3000 points into one key frame, the Sim3 Fuse with 3000 points into 20 key frames
               as one batch -- that row beside pgorb_fuse_batch_device at the same shape --; beside each the wall clock of the
               sequential Python reference (tests/loop_reference.py, OUR restatement, not ORB-SLAM2) for ONE problem, whose results
               the GPU's must equal.  --loop-only runs these rows alone

  tracking     Tracking::SearchLocalPoints (Tracking.cc:1134-1184) as ONE batched resident call with the projection on the device
               (pgorb_search_local_points_batch_device): 127 pairs at 1080p bounds, 2000 keypoints a frame, 3000 local points of a
               resident table; beside it pgorb_search_by_projection_points_batch_device at the same shape, which starts from the
               projections, and the host front part that call needs first: isInFrustum for every point as vectorised numpy on one
               core (OUR restatement, not ORB-SLAM2), the descriptor gather and the upload of the seven arrays, wall clock.  The
               two device calls must assign the same points.  --track-only runs these rows alone

  pose         Optimizer::PoseOptimization (Optimizer.cc:239-451) on the device (pgorb_pose_optimization, csrc/pose_opt.hip): the
               single call at 300 edges of 2000 keypoints (wall clock, staging included) and the batched resident call at 128
               problems x 300 edges and x 2000 edges (HIP events); beside them the wall clock of the sequential Python reference
               of the tests (tests/pose_reference.py, OUR restatement on one core, NOT g2o) for ONE such problem.  There is no
               g2o build to hold these times against and no earlier path in this library.  --pose-only runs these rows alone

  sim3         Sim3Solver (Sim3Solver.cc:37-423) on the device (pgorb_sim3_solver, csrc/sim3.hip): one loop candidate through the
               single call (wall clock, staging included) and 16 candidates in one batched resident call (HIP events), each 150
               correspondences (30 % outliers) and a window of 300 iterations, all of which the device evaluates whenever the
               stop rule would have returned; beside them the wall clock of the sequential Python reference of the tests
               (tests/sim3_reference.py, OUR restatement on one core, NOT ORB-SLAM2: it needs OpenCV, which cannot be built here)
               run to ITS end, which is the stop rule's.  No CPU figure exists to set a target against.  --sim3-only runs these
               rows alone

  pnp          PnPsolver (PnPsolver.cc:67-950) on the device (pgorb_pnp_solver, csrc/pnp.hip): one relocalisation candidate through the
               single call (wall clock, staging included) and 16 candidates in one batched resident call (HIP events), each 150
               correspondences (30 % outliers) with relocalisation's parameters, so a window of 35 iterations, all of which the
               device evaluates whenever the stop rule would have returned; beside them the wall clock of the sequential Python
               reference of the tests (tests/pnp_reference.py, OUR restatement on one core, NOT ORB-SLAM2: it needs OpenCV, which
               cannot be built here) run to ITS end, which is the stop rule's.  No CPU figure exists to set a target against.
               --pnp-only runs these rows alone

  optsim3      Optimizer::OptimizeSim3 (Optimizer.cc:1046-1241) on the device (pgorb_optimize_sim3, csrc/optimize_sim3.hip): one loop
               candidate through the single call (wall clock, staging included) and 16 candidates in one batched resident call
               (HIP events), each 150 correspondences (10 % gross outliers, 0.5 pixel noise); beside them the wall clock of the
               sequential Python reference of the tests (tests/optsim3_reference.py, OUR restatement on one core, NOT g2o).  No
               g2o build exists here, so no CPU counterpart exists and no target is set.  --optsim3-only runs these rows alone

  local_ba     Optimizer::LocalBundleAdjustment (Optimizer.cc:453-778) on the device (pgorb_local_bundle_adjustment_batch_device,
               csrc/local_ba.hip): one window of 20 local and 20 fixed key frames, 2000 points and 12000 edges (2 % gross outliers,
               0.7 sigma noise), alone and 64 times in one call (HIP events); beside them the wall clock of the dense numpy reference of
               the tests (tests/lba_reference.py, NOT g2o and not a tuned CPU baseline).  No target is set.  --lba-only runs these rows

  essential_graph  Optimizer::OptimizeEssentialGraph (Optimizer.cc:781-1044) on the device (pgorb_optimize_essential_graph_device,
               csrc/essential_graph.hip): ONE ride-shaped graph of 500 key frames -- the spanning tree, four covisibles back, a previous
               loop edge and the new loop's three connections -- over its fixed sequence of launches (HIP events around the call alone);
               beside it the wall clock of the dense numpy reference of the tests (tests/eg_reference.py) on the same shape with 100 key
               frames (it is cubic in the key frames): NOT g2o and not a CPU baseline.  No target is set.  --eg-only runs this row
  global_ba        Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:41-237) on the device (pgorb_global_bundle_adjustment_device,
               csrc/global_ba.hip): ONE ride-shaped map of 500 key frames (about 40 points a key frame over 4 frames, one old loop and
               the new one), and LocalBundleAdjustment's benchmark window (40 key frames, 2000 points, 12 000 edges) through both
               optimisers in the same run, with the time per Levenberg trial.  No target is set.  --gba-only runs these rows
               (profiles/next_tier_gba.txt).
  covisibility     the covisibility graph on the device (csrc/covisibility.hip), HIP events: a whole-map KeyFrame::UpdateConnections
               (KeyFrame.cc:392-482) of ONE ride-shaped map -- 500 key frames x 2000 slots, tracks of 2 to 10 consecutive key frames, every
               key frame in the list, th 15 (pgorb_update_connections_batch_device); its views (pgorb_covisibility_views_device); and
               Tracking::UpdateLocalMap (Tracking.cc:1186-1321) of 128 frames of that map, each tracking a third of one key frame's
               points (pgorb_update_local_map_batch_device).  One row's counters are checked against numpy.  Nobody has measured this
               before and there is no CPU baseline (the Python reference of the tests is not one): no target is set, the rows record what
               was measured.  --covis-only runs these rows alone (profiles/next_tier_covis.txt).
  cullings         local mapping's cullings on the device (csrc/culling.hip), HIP events: LocalMapping::KeyFrameCulling (LocalMapping.cc:634-698,
               with KeyFrame::SetBadFlag) of ONE ride-shaped map -- 200 key frames x 2000 slots, tracks of 2 to 40 consecutive key frames, the
               graph from a whole-map UpdateConnections at th 15, the list of the middle key frame -- against the literal Python reference of the
               tests on one core (NOT ORB-SLAM2, not a tuned baseline), whose records the GPU's must equal; MapPointCulling of 3000 recent
               points; the compaction of the observation lists.  No target is set.  --cull-only runs these rows alone
               (profiles/next_tier_cull.txt).
  loop correction  loop closing's two map rewrites on the device (csrc/loop_correct.hip), HIP events: CorrectLoop's propagation
               (LoopClosing.cc:438-516) over the last key frame of a ride-shaped map and its 30 predecessors, and the map update after
               GlobalBundleAdjustment (:679-742) of the same map with the last 50 key frames made while the adjustment ran.  The parent commit
               has no such path and ORB-SLAM2 cannot be built here, so there is nothing measured to compare against: no target is set, the rows
               record what was measured.  --loop-correct-only runs these rows alone (profiles/next_tier_loop_correct.txt).
  trajectory   the trajectory read-out on the device (csrc/track_pose.hip), HIP events: predict + commit over 8 and 128 trackers next to
               the same hand-off through the host (download, numpy products, upload), and GetTrajectory of 108 000 records over 2 000 key
               frames with 30 % of them culled.  No target is set.  --trajectory-only runs these rows alone (profiles/next_tier_trajectory.txt).

usage: python tools/next_tier_bench.py [--batch 128] [--out profiles/r02_next_tier.txt] [--refresh-only | --place-only | --loop-only | --track-only | --pose-only | --sim3-only | --pnp-only | --optsim3-only | --lba-only | --eg-only | --gba-only | --covis-only | --cull-only | --loop-correct-only | --trajectory-only | --edit-only]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import pilotguru_amd as pg
from pilotguru_amd import vocab as V
from pilotguru_amd.synth import synth_ride
from oracle import orb_oracle

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--out", default="")
ap.add_argument("--features", type=int, default=2000, help="4000 = the initialisation extractor (2 * nFeatures, Tracking.cc:143)")
ap.add_argument("--refresh-only", action="store_true", help="the map-point refresh rows alone (no ride, no vocabulary)")
ap.add_argument("--place-only", action="store_true", help="the place-recognition row alone (no ride, no vocabulary)")
ap.add_argument("--loop-only", action="store_true", help="loop closing's four matchers alone (no ride, no vocabulary)")
ap.add_argument("--track-only", action="store_true", help="the tracking thread's SearchLocalPoints rows alone (no ride, no vocabulary)")
ap.add_argument("--pose-only", action="store_true", help="the pose-optimisation rows alone (no ride, no vocabulary)")
ap.add_argument("--sim3-only", action="store_true", help="the Sim3Solver rows alone (no ride, no vocabulary)")
ap.add_argument("--pnp-only", action="store_true", help="the PnPsolver rows alone (no ride, no vocabulary)")
ap.add_argument("--optsim3-only", action="store_true", help="the OptimizeSim3 rows alone (no ride, no vocabulary)")
ap.add_argument("--lba-only", action="store_true", help="the LocalBundleAdjustment rows alone (no ride, no vocabulary)")
ap.add_argument("--eg-only", action="store_true", help="the OptimizeEssentialGraph row alone (no ride, no vocabulary)")
ap.add_argument("--gba-only", action="store_true", help="the GlobalBundleAdjustment rows alone (no ride, no vocabulary)")
ap.add_argument("--covis-only", action="store_true", help="the covisibility-graph rows alone (no ride, no vocabulary)")
ap.add_argument("--cull-only", action="store_true", help="the culling rows alone (no ride, no vocabulary)")
ap.add_argument("--loop-correct-only", action="store_true", help="the loop-correction rows alone (no ride, no vocabulary); writes "
                "profiles/next_tier_loop_correct.txt unless --out names another file")
ap.add_argument("--edit-only", action="store_true", help="the map-edit rows alone (no ride, no vocabulary); writes profiles/next_tier_map_edit.txt")
ap.add_argument("--trajectory-only", action="store_true", help="the trajectory read-out rows alone (no ride, no vocabulary); writes "
                "profiles/next_tier_trajectory.txt unless --out names another file")
a = ap.parse_args()
w, h, nf, B = 1920, 1080, a.features, a.batch


def timed(fn, reps=9):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def refresh_rows(ext):
    """The map-point refresh: (name, batched GPU ms, replaced path ms = D2H + host loop + H2D, host loop ms, distances, points)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_point_cases as PC
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = []
    for label, nkf, nkeys, npts in (("one key frame's tail", 260, 400, 1500), ("a local-BA-sized set", 260, 2000, 20000)):
        c = PC.random_scene(5, nkf=nkf, nkeys=nkeys, npts=npts, bad_kf_share=0.02)
        pts, pd, pb, st, of, oi, ref = PC.table_arrays(c.points)
        kp = np.stack([k for k, _, _, _ in c.kfs]); ds = np.stack([d for _, d, _, _ in c.kfs])
        poses = np.array([P for _, _, P, _ in c.kfs], pg.KF_POSE_DTYPE)
        kb = np.array([b for _, _, _, b in c.kfs], np.uint8)
        dK, dD, dN = G(kp.view(np.uint8).reshape(nkf, nkeys, 28)), G(ds), G(np.full(nkf, nkeys, np.int32))
        dP, dKB, dPts, dPD, dPB = G(poses.view(np.uint8)), G(kb), G(pts.view(np.uint8)), G(pd), G(pb)
        dS, dF, dI, dR = G(st), G(of), G(oi), G(ref)
        best = torch.empty(npts, dtype=torch.int32, device="cuda"); status = torch.empty(npts, dtype=torch.int32, device="cuda")
        call = lambda: ext._check(ext._L.pgorb_refresh_map_points_batch_device(ext._h, p(dK), p(dD), p(dN), nkf, nkeys, p(dP), p(dKB), npts, p(dPts),
                                  p(dPD), p(dPB), p(dS), p(dF), p(dI), len(of), p(dR), npts, None, 3, p(best), p(status), s))
        t_gpu = timed(call)
        want = PC.run_reference(c)
        assert np.array_equal(status.cpu().numpy(), want[3]) and np.array_equal(best.cpu().numpy(), want[2])
        assert dPD.cpu().numpy().tobytes() == want[1].tobytes() and dPts.cpu().numpy().view(pg.MAP_POINT_DTYPE).tobytes() == want[0].tobytes()
        # what the call replaces for a resident back end: the key frames' descriptors come down, the host loops, the points go up
        t0 = time.perf_counter(); dD.cpu(); dK.cpu(); torch.cuda.synchronize(); t_down = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); PC.run_reference(c); t_loop = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); G(want[0].view(np.uint8)); G(want[1]); torch.cuda.synchronize(); t_up = (time.perf_counter() - t0) * 1e3
        live = [(len(q["obs"]), sum(1 for f, _ in q["obs"] if not c.kfs[f][3])) for q in c.points if not q["bad"]]
        ndist = sum(nc * nc for _, nc in live if nc > 2)
        out.append(("refresh: %s, %d points over %d key frames (longest list %d)" % (label, npts, nkf, max(n for n, _ in live)),
                    t_gpu, t_down + t_loop + t_up, t_loop, ndist, npts))
    return out


def refresh_lines(rows):
    lines = ["# map-point refresh (ComputeDistinctiveDescriptors + UpdateNormalAndDepth), batched resident call, HIP events, median of 9;",
             "# replaced = descriptors and keypoints D2H + the Python restatement on one core (NOT ORB-SLAM2) + points H2D, wall clock",
             "%-86s %10s %12s %12s %14s" % ("call", "GPU ms", "replaced ms", "host loop ms", "Gdistances/s")]
    for name, g, rep, loop, nd, _ in rows:
        lines.append("%-86s %10.3f %12.1f %12.1f %14.2f" % (name, g, rep, loop, nd / g / 1e6))
    return lines


def place_lines(ext, nkf=4096, nwords=1500, nq=64, vocab=50000, ccap=256):
    """The relocalisation candidate query, batched: GPU ms (HIP events, median of 9) beside the C++ comparator's seconds."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import place_comparator as CMP
    rng = np.random.RandomState(12)
    N = nkf + nq
    cap = int(nwords * 1.1) + 1
    ids, val, nb = np.zeros((N, cap), np.uint32), np.zeros((N, cap), np.float64), np.zeros(N, np.int32)
    pool = vocab // 8                                       # half of every vector's words come from a small pool: dense sharing
    for f in range(N):
        n = int(rng.randint(int(nwords * 0.9), cap))
        w = np.unique(np.concatenate([rng.randint(0, pool, n // 2), rng.randint(0, vocab, n - n // 2)]))
        v = rng.uniform(0.05, 1.0, len(w))
        nb[f] = len(w); ids[f, :len(w)] = w; val[f, :len(w)] = v / v.sum()
    in_db = np.zeros(N, np.uint8); in_db[:nkf] = 1
    neigh = np.full((N, 10), -1, np.int32)
    neigh[:nkf] = rng.randint(0, nkf, (nkf, 10))
    queries = np.arange(nkf, N, dtype=np.int32)
    state = rng.uniform(0, 0.05, N).astype(np.float32)
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dI, dV, dN, dDb, dNe, dQ, dS = G(ids.view(np.int32)), G(val), G(nb), G(in_db), G(neigh), G(queries), G(state)
    cand = torch.full((nq, ccap), -1, dtype=torch.int32, device="cuda"); ncand = torch.empty(nq, dtype=torch.int32, device="cuda")
    common = torch.empty((nq, N), dtype=torch.int32, device="cuda"); score = torch.empty((nq, N), dtype=torch.float32, device="cuda")
    stats = torch.empty((nq, 3), dtype=torch.int32, device="cuda")
    call = lambda: ext._check(ext._L.pgorb_detect_relocalization_candidates_batch_device(ext._h, p(dI), p(dV), p(dN), N, cap, p(dDb), p(dNe), p(dQ), nq,
                              p(dS), p(cand), ccap, p(ncand), p(common), p(score), p(stats), s))
    t_gpu = timed(call)
    start = np.zeros(N + 1, np.int32); start[1:] = np.cumsum(nb)
    mask = np.arange(cap)[None, :] < nb[:, None]
    nstart = np.zeros(N + 1, np.int32); nstart[1:nkf + 1] = 10 * np.arange(1, nkf + 1); nstart[nkf + 1:] = 10 * nkf
    c_cand, c_ncand, c_common, c_score, c_stats, sec = CMP.run(False, start, ids[mask], val[mask], in_db, nstart, neigh[:nkf].reshape(-1), queries,
                                                                state, ccap=ccap)
    g_ncand = ncand.cpu().numpy()
    assert np.array_equal(g_ncand, c_ncand) and np.array_equal(common.cpu().numpy(), c_common) and np.array_equal(stats.cpu().numpy(), c_stats)
    assert score.cpu().numpy().tobytes() == c_score.tobytes()
    g_cand = cand.cpu().numpy()
    assert all(np.array_equal(g_cand[q, :min(n, ccap)], c_cand[q, :min(n, ccap)]) for q, n in enumerate(c_ncand))
    return ["# place recognition (DetectRelocalizationCandidates), one batched resident call, HIP events, median of 9;",
            "# CPU = the tool's C++ std::map / std::list restatement on one core (NOT ORB-SLAM2), its queries alone, results equal",
            "%-86s %10s %12s %14s" % ("call", "GPU ms", "CPU ms", "candidates"),
            "%-86s %10.3f %12.1f %14d" % ("place: %d key frames of %d words (mean), %d queries, sharing %d, scored %d per query" %
                                          (nkf, int(nb.mean()), nq, int(c_stats[:, 0].mean()), int(c_stats[:, 2].mean())), t_gpu, sec * 1e3,
                                          int(c_ncand.sum()))]


def loop_lines():
    """Loop closing's four matchers, batched: GPU ms (HIP events, median of 9) beside the Python reference's ms for one problem."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fuse_cases as FC
    import loop_cases as LC
    ext = pg.ORBextractor(2000, FC.MC.SCALE, FC.NLEVELS, 20, 7, max_width=640, max_height=480)      # the scale tables of the constructed scenes

    def ref_ms(fn, c):
        t0 = time.perf_counter(); r = fn(c); return r, (time.perf_counter() - t0) * 1e3
    rows = []
    # 1: SearchByBoW(KF, KF), 8 candidate pairs of about 2000 features
    bows = [LC.bow_case(100 + k, n=1500, nodes=300) for k in range(8)]
    got = LC.run_gpu1_batched(bows, ext, timer=timed)
    want, ms = ref_ms(LC.run_ref1, bows[0])
    assert LC.same(want, got[0])
    rows.append(("SearchByBoW(KF, KF): 8 pairs of %d x %d features, %d matches in pair 0" % (len(bows[0].k1[1]), len(bows[0].k2[1]), want[0]), LC.LAST_MS[1], ms))
    # 2: SearchBySim3, 8 pairs
    pairs = [LC.pair_case(100 + k, npts=1800) for k in range(8)]
    got = LC.run_gpu2_batched(pairs, ext, timer=timed)
    want, ms = ref_ms(LC.run_ref2, pairs[0])
    assert LC.same(want, got[0][:2])
    rows.append(("SearchBySim3: 8 pairs of %d x %d features, %d found in pair 0" % (len(pairs[0].slots1), len(pairs[0].slots2), want[0]), LC.LAST_MS[2], ms))
    # 3: SearchByProjection(KF, Scw), 3000 points into one key frame, th = 10
    w = LC.wide_case(21, 3000)
    w10 = LC.Case(w.name, w.kf, w.points, w.slots, w.queries, th=10)
    got = LC.run_gpu_batched([w10], ext, 3, timer=timed)
    want, ms = ref_ms(LC.run_ref3, w10)
    assert LC.same(want, got[0][:-1])
    rows.append(("SearchByProjection(KF, Scw): %d points into one key frame of %d keypoints, %d matches" % (3000, len(w.slots), want[0]), LC.LAST_MS[3], ms))
    # 4: the Sim3 Fuse, 3000 points into 20 key frames as one batch (th = 4), every slot empty; beside it Fuse(KF, points) at the same shape
    e = LC.Case(w.name, w.kf, w.points, np.full(len(w.slots), -1, np.int32), w.queries, th=4)
    got = LC.run_gpu_batched([e] * 20, ext, 4, timer=timed)
    want, ms = ref_ms(LC.run_ref4, e)
    assert all(LC.same(want, g[:-1]) for g in got)
    rows.append(("Fuse(KF, Scw): %d points into 20 key frames of %d keypoints as one batch, %d fused each" % (3000, len(w.slots), want[0]), LC.LAST_MS[4], ms))
    # pgorb_fuse_batch_device on the same 20 problems (no observations, every slot empty, th = 4): it also runs the chi-square test
    B, n, nq = 20, len(w.slots), len(w.queries)
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pts, pd, pb, st, ob = FC.table_arrays([dict(q, obs=[]) for q in w.points])
    kid, k, d, P, b = w.kf
    dK = G(np.tile(k.view(np.uint8).reshape(1, n, 28), (B, 1, 1))); dD = G(np.tile(d.reshape(1, n, 32), (B, 1, 1)))
    dN = G(np.full(B, n, np.int32)); gs = torch.zeros((B, 3073), dtype=torch.int32, device="cuda"); gi = torch.zeros((B, n), dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(dK), p(dN), B, n, *b, p(gs), p(gi), s))
    dKf, dId, dP = G(np.arange(B, dtype=np.int32)), G(np.arange(B, dtype=np.int64)), G(np.tile(np.array(P, pg.KF_POSE_DTYPE).reshape(1).view(np.uint8), (B, 1)))
    dPts, dPD, dPB, dSt, dOb = G(pts.view(np.uint8)), G(pd), G(pb), G(st), torch.zeros(1, dtype=torch.int64, device="cuda")
    dNq, dQ = G(np.full(B, nq, np.int32)), G(np.tile(np.array(w.queries, np.int32), (B, 1)))
    act = torch.empty((B, nq), dtype=torch.int32, device="cuda"); nfu = torch.empty(B, dtype=torch.int32, device="cuda")
    fuse = lambda: ext._check(ext._L.pgorb_fuse_batch_device(ext._h, p(dK), p(dD), p(dN), n, p(gs), p(gi), p(dKf), B, p(dId), p(dP), *b, None,
                              len(pts), p(dPts), p(dPD), p(dPB), p(dSt), p(dOb), nq, p(dNq), p(dQ), 4.0, p(act), None, None, None, p(nfu), s))
    t_fuse = timed(fuse)
    rows.append(("   beside it Fuse(KF, points), pgorb_fuse_batch_device, the same 20 problems, %d fused each" % int(nfu[0]), t_fuse, float("nan")))
    lines = ["# loop closing's matchers, batched resident calls, HIP events, median of 9;",
             "# reference = tests/loop_reference.py (Python, one core, NOT ORB-SLAM2) for ONE problem of the batch, wall clock, results equal",
             "%-104s %10s %14s" % ("call", "GPU ms", "reference ms")]
    return lines + ["%-104s %10.3f %14.1f" % r for r in rows]


def track_lines(npairs=127, cap=2000, npts=3000):
    """SearchLocalPoints, batched and resident, with the front part on the device; beside it the matcher that starts from the
    projections and the host front part it needs."""
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    rng = np.random.RandomState(9)
    f, cx, cy = 1400.0, w / 2.0, h / 2.0
    bnd = (0.0, float(w), 0.0, float(h))
    sf = ext.GetScaleFactors()
    # the table: points on a slab 4 .. 9 in front of the first camera, seen head-on; the cameras move sideways, 0.004 a frame
    z = rng.uniform(4.0, 9.0, npts)
    pts = np.zeros(npts, pg.MAP_POINT_DTYPE)
    pts["pos"] = np.stack([(rng.uniform(-80, w + 330, npts) - cx) * z / f, (rng.uniform(-60, h + 60, npts) - cy) * z / f, z], 1)
    pts["normal"] = [0.0, 0.0, 1.0]
    pts["max_distance"] = (z * sf[rng.randint(1, 8, npts)]).astype(np.float32)
    pts["min_distance"] = pts["max_distance"] / sf[7]
    pdesc = rng.randint(0, 256, (npts, 32)).astype(np.uint8)
    pbad = (rng.uniform(size=npts) < 0.02).astype(np.uint8)
    pobs = (rng.uniform(size=npts) > 0.1).astype(np.uint8)
    B_ = npairs + 1
    poses = np.zeros(B_, pg.KF_POSE_DTYPE)
    kp = np.zeros((B_, cap), pg.KEYPOINT_DTYPE)
    ds = rng.randint(0, 256, (B_, cap, 32)).astype(np.uint8)
    slots = np.full((npairs, cap), -1, np.int32)
    for k in range(B_):
        c = np.array([0.004 * k, 0.002 * k, 0.0])
        poses[k] = pg.kf_pose(np.hstack([np.eye(3), -c[:, None]]), c, f, f, cx, cy)
        pc = pts["pos"].astype(np.float64) - c
        u, v = f * pc[:, 0] / pc[:, 2] + cx, f * pc[:, 1] / pc[:, 2] + cy
        vis = np.flatnonzero((u > 1) & (u < w - 1) & (v > 1) & (v < h - 1))
        own = rng.permutation(vis)[:int(cap * 0.75)]                      # three quarters of the keypoints sit on a point's projection
        m = len(own)
        kp[k]["x"], kp[k]["y"] = rng.uniform(0, w - 1, cap), rng.uniform(0, h - 1, cap)
        kp[k]["x"][:m], kp[k]["y"][:m] = u[own] + rng.uniform(-1, 1, m), v[own] + rng.uniform(-1, 1, m)
        kp[k]["octave"] = rng.randint(0, 8, cap)
        lvl = np.clip(np.ceil(np.log(pts["max_distance"][own] / np.linalg.norm(pc[own], axis=1)) / np.log(1.2)), 0, 7).astype(np.int32)
        kp[k]["octave"][:m] = lvl
        kp[k]["angle"], kp[k]["size"] = rng.uniform(0, 360, cap), 31.0
        flip = rng.randint(0, 256, (m, 3))                                # the keypoint's descriptor: the point's with up to 24 bits flipped
        d = pdesc[own].copy()
        for j in range(3):
            d[np.arange(m), flip[:, j] % 32] ^= (flip[:, j] & 0xFF).astype(np.uint8)
        ds[k, :m] = d
        if k >= 1:
            slots[k - 1, :m:5] = own[::5]                                 # a fifth of them already hold their point (tracked from the last frame)
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dK, dD, dN = G(kp.view(np.uint8).reshape(B_, cap, 28)), G(ds), G(np.full(B_, cap, np.int32))
    gs = torch.empty((B_, 3073), dtype=torch.int32, device="cuda"); gi = torch.empty((B_, cap), dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(dK), p(dN), B_, cap, *bnd, p(gs), p(gi), s))
    pairF = torch.arange(1, B_, dtype=torch.int32, device="cuda")
    dPose = G(poses[1:].view(np.uint8).reshape(npairs, -1))
    dPts, dPD, dPB, dPO, dSl = G(pts.view(np.uint8).reshape(npts, 32)), G(pdesc), G(pbad), G(pobs), G(slots)
    q = np.stack([rng.permutation(npts) for _ in range(npairs)]).astype(np.int32)
    dQ, dNq = G(q), G(np.full(npairs, npts, np.int32))
    I32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")
    F32 = lambda *sh: torch.empty(sh, dtype=torch.float32, device="cuda")
    iv = torch.empty((npairs, npts), dtype=torch.uint8, device="cuda")
    px, py, lv, vc = F32(npairs, npts), F32(npairs, npts), I32(npairs, npts), F32(npairs, npts)
    kpo, ntm, asg, nm = I32(npairs, cap), I32(npairs), I32(npairs, cap), I32(npairs)
    new = lambda: ext._check(ext._L.pgorb_search_local_points_batch_device(ext._h, p(dK), p(dD), p(dN), cap, p(gs), p(gi), p(pairF), npairs, *bnd,
                             p(dPose), p(dSl), npts, p(dPts), p(dPD), p(dPB), p(dPO), npts, p(dNq), p(dQ), None, 0.5, 1.0, 0.8, p(iv), p(px),
                             p(py), p(lv), p(vc), p(kpo), p(ntm), p(asg), p(nm), s))
    t_new = timed(new)
    # the matcher that starts from the projections, fed with what the new call computed (its front part's outputs)
    has = ((kpo >= 0) & (dPO[kpo.clamp(min=0).long()] != 0)).to(torch.uint8).contiguous()
    qd, qo = dPD[dQ.long()].contiguous(), dPO[dQ.long()].contiguous()
    asg2, nm2 = I32(npairs, cap), I32(npairs)
    old = lambda: ext._check(ext._L.pgorb_search_by_projection_points_batch_device(ext._h, p(dK), p(dD), p(dN), cap, p(gs), p(gi), p(pairF), npairs,
                             *bnd, p(has), npts, p(dNq), p(iv), p(px), p(py), p(lv), p(vc), p(qd), p(qo), 1.0, 0.8, p(asg2), p(nm2), s))
    t_old = timed(old)
    assert torch.equal(asg, asg2) and torch.equal(nm, nm2)
    # the host front part that call needs first, for ONE pair: isInFrustum vectorised in float32 numpy, the gather, the upload
    def host_front(j):
        P_, T_ = pts["pos"][q[j]], poses[j + 1]["Tcw"].reshape(3, 4)
        pc = P_ @ T_[:, :3].T + T_[:, 3]
        with np.errstate(all="ignore"):
            invz = np.float32(1) / pc[:, 2]
            u, v = np.float32(f) * pc[:, 0] * invz + np.float32(cx), np.float32(f) * pc[:, 1] * invz + np.float32(cy)
            po = P_ - poses[j + 1]["Ow"]
            dist = np.sqrt((po.astype(np.float64) ** 2).sum(1)).astype(np.float32)
            vcos = ((po.astype(np.float64) * pts["normal"][q[j]]).sum(1) / dist).astype(np.float32)
            mx, mn = pts["max_distance"][q[j]], pts["min_distance"][q[j]]
            lvl = np.clip(np.ceil(np.log(mx / dist) / np.log(np.float32(1.2))), 0, 7).astype(np.int32)
        ok = (pc[:, 2] >= 0) & (u >= 0) & (u <= w) & (v >= 0) & (v <= h) & (dist >= np.float32(0.8) * mn) & (dist <= np.float32(1.2) * mx) & \
            (vcos >= 0.5) & (pbad[q[j]] == 0)
        arrs = [ok.astype(np.uint8), u, v, lvl, vcos, pdesc[q[j]], pobs[q[j]]]
        return [G(x) for x in arrs]
    host_front(0); torch.cuda.synchronize()
    ts = []
    for j in range(9):
        t0 = time.perf_counter(); host_front(j); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    t_host = float(np.median(ts))
    nin, nmm = float(ntm.float().mean()), float(nm.float().mean())
    head = "%d pairs x %d keypoints x %d local points (%d in view, %d matches a pair)" % (npairs, cap, npts, nin, nmm)
    return ["# the tracking thread's SearchLocalPoints, batched resident calls, HIP events, median of 9; host front part = isInFrustum of one pair's",
            "# points as vectorised numpy on one core (OUR restatement, NOT ORB-SLAM2) + descriptor gather + upload of the 7 arrays, wall clock, median of 9",
            "%-118s %10s %12s" % ("call", "GPU ms", "GPU ms/pair"),
            "%-118s %10.3f %12.4f" % ("search_local_points (front part on the device): " + head, t_new, t_new / npairs),
            "%-118s %10.3f %12.4f" % ("search_by_projection_points (starts from the projections), the same shape and arrays", t_old, t_old / npairs),
            "%-118s %10.3f %12.4f" % ("   the host front part search_by_projection_points needs first: ms per pair, x %d pairs" % npairs, t_host * npairs, t_host)]


def pose_lines(npairs=128, cap=2000):
    """PoseOptimization: the single call and the batched resident call, beside the Python reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pose_cases as PC
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = ["# Optimizer::PoseOptimization on the device; single call = wall clock with staging, median of 9; batched resident call = HIP events, median of 9;",
           "# reference = tests/pose_reference.py for ONE problem, wall clock: OUR restatement in numpy on one core, NOT g2o (no g2o build exists here to time)",
           "%-96s %10s %14s %16s" % ("call", "GPU ms", "GPU ms/problem", "reference ms (1)")]
    for edges in (300, cap):
        cs = [PC.scene("bench", 1000 + j, edges, cap, noise=0.5, outliers=0.2, extra_points=0) for j in range(8)]
        t0 = time.perf_counter(); ref = PC.run_reference(cs[0]); t_ref = (time.perf_counter() - t0) * 1e3
        if edges == 300:
            ts = []
            for j in range(10):
                t0 = time.perf_counter(); got = PC.run_gpu(cs[0], ext); ts.append((time.perf_counter() - t0) * 1e3)
            assert got["ret"] == ref["ret"] and np.array_equal(got["outlier"], ref["outlier"])
            t1 = float(np.median(ts[1:]))
            out.append("%-96s %10.3f %14.4f %16.1f" % ("pose_optimization (single call): %d edges of %d keypoints, %d inliers" % (edges, cap, ref["ret"]), t1, t1, t_ref))
        # the batch: 128 problems, 8 distinct scenes repeated, each its own frame and table slice
        kp = np.zeros((npairs, cap), pg.KEYPOINT_DTYPE)
        slots = np.zeros((npairs, cap), np.int32)
        poses = np.zeros(npairs, pg.KF_POSE_DTYPE)
        pts = np.concatenate([PC.table(c.points) for c in cs])
        off = np.cumsum([0] + [len(c.points) for c in cs])
        for j in range(npairs):
            c = cs[j % 8]
            kp[j] = PC.keypoints(c.keys_xy, c.octaves)
            slots[j] = np.where(c.kp_point >= 0, c.kp_point + off[j % 8], -1)
            poses[j] = PC.pose_record(c.pose)
        dK, dN, dS = G(kp.view(np.uint8).reshape(npairs, cap, 28)), G(np.full(npairs, cap, np.int32)), G(slots)
        dP, dT = G(poses.view(np.uint8).reshape(npairs, -1)), G(pts.view(np.uint8).reshape(len(pts), 32))
        oP = torch.empty((npairs, pg.KF_POSE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        oF = torch.empty((npairs, cap), dtype=torch.uint8, device="cuda")
        oK, oI, oN = (torch.empty(sh, dtype=torch.int32, device="cuda") for sh in ((npairs, cap), (npairs, 8), (npairs,)))
        run = lambda: ext._check(ext._L.pgorb_pose_optimization_batch_device(ext._h, p(dK), p(dN), cap, None, npairs, p(dP), p(dS), len(pts), p(dT), None, 1,
                                 p(oP), p(oF), p(oK), None, None, p(oI), p(oN), s))
        t = timed(run)
        assert int(oN[0]) == ref["ret"] and torch.equal(oN[:8], oN[8:16])
        info = oI.cpu().numpy()
        out.append("%-96s %10.3f %14.4f %16.1f" % ("pose_optimization_batch_device: %d problems x %d edges of %d keypoints (%.1f iterations, %.1f trials a problem)" % (
            npairs, edges, cap, info[:, 2:6].sum(1).mean(), info[:, 6].mean()), t, t / npairs, t_ref))
    return out


def sim3_lines(npairs=16, ngood=105, nout=45):
    """Sim3Solver: the single call and the batched resident call, beside the Python reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sim3_cases as SC
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    cs = [SC.scene("bench%d" % j, 3000 + j, ngood, nout, s=1.0 + 0.05 * j, noise=0.3) for j in range(npairs)]
    N = ngood + nout
    t0 = time.perf_counter(); ref = SC.run_reference(cs[0]); t_ref = (time.perf_counter() - t0) * 1e3
    ts = []
    for j in range(10):
        t0 = time.perf_counter(); got = SC.run_gpu(cs[0], ext); ts.append((time.perf_counter() - t0) * 1e3)
    assert got["ret"] == ref["ret"] and np.array_equal(got["inlier"], ref["inlier"]) and got["cap"] == 300
    t1 = float(np.median(ts[1:]))
    res = {}
    run = lambda: res.__setitem__("r", SC.run_gpu_batch(cs, ext, N))
    run()
    # the batched call alone, on resident arrays: the runner's uploads are outside the events
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nfr = 2 * npairs
    kp = np.zeros((nfr, N), pg.KEYPOINT_DTYPE); slots = np.full((nfr, N), -1, np.int32); m12 = np.full((npairs, N), -1, np.int32)
    poses = np.zeros(nfr, pg.KF_POSE_DTYPE); draws = np.zeros((npairs, 300, 3), np.uint32)
    base, tabs = 0, []
    for j, c in enumerate(cs):
        kp[2 * j, :c.n1] = SC.keypoints(c.octaves1)[:c.n1]; kp[2 * j + 1, :c.n2] = SC.keypoints(c.octaves2)[:c.n2]
        slots[2 * j, :c.n1] = c.kf_point1 + base; slots[2 * j + 1, :c.n2] = c.kf_point2 + base
        m12[j, :c.n1] = c.matches12; poses[2 * j], poses[2 * j + 1] = SC.pose_record(c.pose1), SC.pose_record(c.pose2)
        draws[j] = c.draws; tabs.append(SC.table(c.points)[:len(c.points)]); base += len(c.points)
    tab = np.concatenate(tabs)
    dK, dN, dP, dS, dM = G(kp.view(np.uint8).reshape(nfr, N, 28)), G(np.full(nfr, N, np.int32)), G(poses.view(np.uint8).reshape(nfr, -1)), G(slots), G(m12)
    dT, dD = G(tab.view(np.uint8).reshape(len(tab), 32)), G(draws.view(np.int32))
    d1, d2 = G(np.arange(0, nfr, 2, dtype=np.int32)), G(np.arange(1, nfr, 2, dtype=np.int32))
    out_t = None
    def batched():
        nonlocal out_t
        out_t = pg.Sim3Solver.iterate_batch_device(ext, dK, dN, N, d1, d2, dP, dS, dM, len(tab), dT, None, dD, 0.99, 20, 300, 300)
    t = timed(batched)
    ninl = out_t["ninliers"].cpu().numpy()
    assert [int(x) for x in ninl] == [r["ret"] for r in res["r"]] and int(ninl[0]) == ref["ret"]
    its = out_t["info"].cpu().numpy()[:, 3]
    return ["# Sim3Solver on the device; single call = wall clock with staging, median of 9; batched resident call = HIP events, median of 9 (its nine",
            "# output arrays are allocated inside the timed call); every call evaluates its whole window of 300 iterations; reference = tests/sim3_reference.py",
            "# for ONE candidate run to the stop rule's return, wall clock: OUR restatement in numpy on one core, NOT ORB-SLAM2's Sim3Solver, which needs",
            "# OpenCV and cannot be built here.  No CPU figure exists to set a target against; none is set.",
            "%-110s %10s %16s %16s" % ("call", "GPU ms", "GPU ms/candidate", "reference ms (1)"),
            "%-110s %10.3f %16.4f %16.1f" % ("sim3_solver (single call): %d correspondences, 300 iterations evaluated, returned at iteration %d with %d inliers" % (
                N, got["its_after"] - 1, got["ret"]), t1, t1, t_ref),
            "%-110s %10.3f %16.4f %16.1f" % ("sim3_solver_batch_device: %d candidates x 300 iterations x %d correspondences (returned after %.1f iterations on average)" % (
                npairs, N, its.mean()), t, t / npairs, t_ref)]


def pnp_lines(npairs=16, ngood=105, nout=45):
    """PnPsolver: the single call and the batched resident call, beside the Python reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pnp_cases as PC
    import pnp_reference as PR
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    cs = [PC.scene("bench%d" % j, 4000 + j, ngood, nout, noise=0.3) for j in range(npairs)]
    N = ngood + nout
    rec = PC.records(cs[0])
    t0 = time.perf_counter()
    ref = PC.finish(cs[0], rec, PR.iterate_literal(rec, cs[0].cam, PC.ref_params(cs[0]), cs[0].draws, PC.state_of(cs[0], rec)))
    t_ref = (time.perf_counter() - t0) * 1e3
    ts = []
    for j in range(10):
        t0 = time.perf_counter(); got = PC.run_gpu(cs[0], ext); ts.append((time.perf_counter() - t0) * 1e3)
    assert got["ret"] == ref["ninliers"] and np.array_equal(got["inlier"], ref["inlier"]) and got["cap"] == 35 and got["status"] == ref["status"]
    t1 = float(np.median(ts[1:]))
    res = PC.run_gpu_batch(cs, ext, N)
    # the batched call alone, on resident arrays: the runner's uploads are outside the events
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    W = PC.window_cap(cs[0].params)
    kp = np.zeros((npairs, N), pg.KEYPOINT_DTYPE); slots = np.full((npairs, N), -1, np.int32)
    cams = np.zeros(npairs, pg.KF_POSE_DTYPE); draws = np.zeros((npairs, W, 4), np.uint32)
    base, tabs = 0, []
    for j, c in enumerate(cs):
        kp[j, :c.n] = PC.keypoints(c)[:c.n]; slots[j, :c.n] = c.kp_point + base
        cams[j], draws[j] = PC.camera_record(c.cam), c.draws
        tabs.append(PC.table(c.points)[:len(c.points)]); base += len(c.points)
    tab = np.concatenate(tabs)
    dK, dN, dC, dS = G(kp.view(np.uint8).reshape(npairs, N, 28)), G(np.full(npairs, N, np.int32)), G(cams.view(np.uint8).reshape(npairs, -1)), G(slots)
    dT, dD = G(tab.view(np.uint8).reshape(len(tab), 32)), G(draws.view(np.int32))
    out_t = None
    def batched():
        nonlocal out_t
        out_t = pg.PnPsolver.iterate_batch_device(ext, dK, dN, N, None, npairs, dC, dS, len(tab), dT, None, dD)
    t = timed(batched)
    ninl = out_t["ninliers"].cpu().numpy()
    assert [int(x) for x in ninl] == [r["ret"] for r in res] and int(ninl[0]) == ref["ninliers"]
    its = out_t["info"].cpu().numpy()[:, 4]
    return ["# PnPsolver on the device; single call = wall clock with staging, median of 9; batched resident call = HIP events, median of 9 (its five",
            "# output arrays are allocated inside the timed call); every call evaluates its whole window of 35 iterations; reference = tests/pnp_reference.py",
            "# for ONE candidate run to the stop rule's return, wall clock: OUR restatement in Python on one core, NOT ORB-SLAM2's PnPsolver, which needs",
            "# OpenCV and cannot be built here.  No CPU figure exists to set a target against; none is set.",
            "%-110s %10s %16s %16s" % ("call", "GPU ms", "GPU ms/candidate", "reference ms (1)"),
            "%-110s %10.3f %16.4f %16.1f" % ("pnp_solver (single call): %d correspondences, 35 iterations evaluated, returned at iteration %d with %d inliers" % (
                N, got["returned"], got["ret"]), t1, t1, t_ref),
            "%-110s %10.3f %16.4f %16.1f" % ("pnp_solver_batch_device: %d candidates x 35 iterations x %d correspondences (returned after %.1f iterations on average)" % (
                npairs, N, its.mean()), t, t / npairs, t_ref)]


def optsim3_lines(npairs=16, ncorr=150, nout=15):
    """OptimizeSim3: the single call and the batched resident call, beside the Python reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import optsim3_cases as OC
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    cs = [OC.scene("bench%d" % j, 4000 + j, ncorr, nout, s=1.0 + 0.05 * j, noise=0.5, octaves="mixed") for j in range(npairs)]
    t0 = time.perf_counter(); ref = OC.run_reference(cs[0]); t_ref = (time.perf_counter() - t0) * 1e3
    ts = []
    for j in range(10):
        t0 = time.perf_counter(); got = OC.run_gpu(cs[0], ext); ts.append((time.perf_counter() - t0) * 1e3)
    assert got["ret"] == ref["ret"] and np.array_equal(got["matches12_out"], ref["matches12_out"])
    t1 = float(np.median(ts[1:]))
    res = OC.run_gpu_batch(cs, ext)
    # the batched call alone, on resident arrays
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nfr, cap = 2 * npairs, max(max(c.n1, c.n2) for c in cs)
    kp = np.zeros((nfr, cap), pg.KEYPOINT_DTYPE); slots = np.full((nfr, cap), -1, np.int32); m12 = np.full((npairs, cap), -1, np.int32)
    poses = np.zeros(nfr, pg.KF_POSE_DTYPE); ests = np.zeros(npairs, pg.SIM3_ESTIMATE_DTYPE); ns = np.zeros(nfr, np.int32)
    base, tabs = 0, []
    for j, c in enumerate(cs):
        kp[2 * j, :c.n1] = OC.keypoints(c.keys1, c.octaves1); kp[2 * j + 1, :c.n2] = OC.keypoints(c.keys2, c.octaves2)
        slots[2 * j, :c.n1] = np.where(c.kf_point1 >= 0, c.kf_point1 + base, -1); slots[2 * j + 1, :c.n2] = np.where(c.kf_point2 >= 0, c.kf_point2 + base, -1)
        m12[j, :c.n1] = c.matches12; poses[2 * j], poses[2 * j + 1] = OC.pose_record(c.pose1), OC.pose_record(c.pose2)
        ests[j] = OC.estimate_record(c.estimate)[0]; ns[2 * j], ns[2 * j + 1] = c.n1, c.n2
        tabs.append(OC.table(c.points)[:len(c.points)]); base += len(c.points)
    tab = np.concatenate(tabs)
    dK, dN, dP, dS, dM = G(kp.view(np.uint8).reshape(nfr, cap, 28)), G(ns), G(poses.view(np.uint8).reshape(nfr, -1)), G(slots), G(m12)
    dT, dE = G(tab.view(np.uint8).reshape(len(tab), 32)), G(ests.view(np.uint8).reshape(npairs, -1))
    d1, d2 = G(np.arange(0, nfr, 2, dtype=np.int32)), G(np.arange(1, nfr, 2, dtype=np.int32))
    out_t = None
    def batched():
        nonlocal out_t
        out_t = pg.Optimizer.OptimizeSim3_batch_device(ext, dK, dN, cap, d1, d2, dP, dS, dM, len(tab), dT, None, dE, 10.0, False)
    t = timed(batched)
    nin = out_t["nin"].cpu().numpy()
    assert [int(x) for x in nin] == [r["ret"] for r in res] and int(nin[0]) == ref["ret"]
    info = out_t["info"].cpu().numpy()
    return ["# Optimizer::OptimizeSim3 on the device; single call = wall clock with staging, median of 9; batched resident call = HIP events, median of 9 (its",
            "# seven output arrays are allocated inside the timed call); reference = tests/optsim3_reference.py for ONE candidate, wall clock: OUR restatement",
            "# in numpy on one core, NOT g2o.  No g2o build exists here to time, so no CPU counterpart exists; no target is set.",
            "%-118s %10s %16s %16s" % ("call", "GPU ms", "GPU ms/candidate", "reference ms (1)"),
            "%-118s %10.3f %16.4f %16.1f" % ("optimize_sim3 (single call): %d correspondences, %d removed, %d + %d iterations, %d + %d trials, %d inliers" % (
                got["ncorr"], got["nbad"], got["iterations"][0], got["iterations"][1], got["trials"][0], got["trials"][1], got["ret"]), t1, t1, t_ref),
            "%-118s %10.3f %16.4f %16.1f" % ("optimize_sim3_batch_device: %d candidates x %d correspondences (%.1f iterations, %.1f trials a candidate)" % (
                npairs, ncorr, (info[:, 3] + info[:, 5]).mean(), (info[:, 4] + info[:, 6]).mean()), t, t / npairs, t_ref)]


def lba_lines(nwin=64, nlocal=20, nfixed=20, npts=2000, nobs=6):
    """LocalBundleAdjustment: one window and a batch of equal windows in the resident call, beside the Python reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lba_cases as LC
    import lba_reference as LR
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    P = LC.window("bench", 7000, nlocal, nfixed, npts, nobs=nobs, noise=0.7, outliers=npts * nobs // 50, far=20)
    LC._cache["bench"] = (P, 2)
    t0 = time.perf_counter(); ref = LR.local_bundle_adjustment(P, 2); t_ref = (time.perf_counter() - t0) * 1e3
    one, many = LC.Batch(["bench"]), LC.Batch(["bench"] * nwin)
    r1 = LC.run_gpu_batch(one, ext, time_reps=5)[0]
    rn = LC.run_gpu_batch(many, ext, time_reps=5)
    assert list(r1["info"]) == list(ref["info"]) and r1["ret"] == ref["ret"] and np.array_equal(r1["erase"], ref["erase"])
    assert all(r["table_bytes"] == r1["table_bytes"] and r["pose_bytes"] == r1["pose_bytes"] for r in rn)
    i = r1["info"]
    scene = "%d local + %d fixed key frames, %d points, %d edges, %d erased, %d + %d iterations, %d + %d trials" % (
        i[3], i[4], i[2], i[1], r1["ret"], i[5], i[7], i[6], i[8])
    return ["# Optimizer::LocalBundleAdjustment on the device, resident batched call, HIP events around the call alone (its eight output arrays are",
            "# allocated inside it), median of 5; one workgroup per window.  reference = tests/lba_reference.py for ONE window, wall clock: OUR dense",
            "# restatement in numpy on one core, NOT g2o and not a tuned CPU baseline.  No g2o build exists here to time; no target is set.",
            "%-132s %10s %14s %16s" % ("call", "GPU ms", "GPU ms/window", "reference ms (1)"),
            "%-132s %10.3f %14.4f %16.1f" % ("local_ba, 1 window: " + scene, one.ms, one.ms, t_ref),
            "%-132s %10.3f %14.4f %16.1f" % ("local_ba, %d windows of that scene in one call" % nwin, many.ms, many.ms / nwin, t_ref)]


def eg_lines(nkf=500, nref=100, back=4):
    """OptimizeEssentialGraph: one graph in the resident call, beside the Python reference of the tests on a smaller graph of that shape."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import warnings
    import eg_cases as EC
    import eg_reference as ER
    warnings.simplefilter("ignore")

    def graph(n):
        le = [[] for _ in range(n)]
        le[3 * n // 5], le[n // 10] = [n // 10], [3 * n // 5]
        return EC.build(n, 77, covis_back=back, loop_edges=le, loop_conn=[(n - 1, 0, 60), (n - 1, 1, 110), (n - 2, 0, 120)])
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    small = graph(nref)
    t0 = time.perf_counter(); ref = ER.optimize_essential_graph(small); t_ref = (time.perf_counter() - t0) * 1e3
    c = graph(nkf)
    dev = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy()).cuda()
    i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32).reshape(-1).copy()).cuda()
    T = dict(id=torch.from_numpy(c["kf_id"].astype(np.int64)).cuda(), pose=dev(c["pose"]), par=i32(c["parent"]), lc=i32(c["loop_conn"]),
             ls=i32(c["loop_edge_start"]), le=i32(c["loop_edge"]), cs=i32(c["covis_start"]), cv=i32(c["covis"]), cw=i32(c["covis_weight"]),
             ref=i32(c["point_ref_kf"]), kb=dev(c["kf_bad"]), pb=dev(c["point_bad"]), hc=dev(c["has_corrected"]), co=dev(c["corrected"]),
             hn=dev(c["has_non_corrected"]), no=dev(c["non_corrected"]))
    pts0 = dev(c["points"])
    ms, out = [], None
    for _ in range(6):
        pts = pts0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pg.Optimizer.OptimizeEssentialGraph_device(ext, T["id"], T["pose"], c["loop_kf"], c["cur_kf"], T["par"], T["lc"], T["ls"], T["le"], T["cs"],
                                                         T["cv"], T["cw"], len(c["points"]), pts, T["ref"], d_kf_bad=T["kb"], d_point_bad=T["pb"],
                                                         d_has_corrected=T["hc"], d_corrected=T["co"], d_has_non_corrected=T["hn"],
                                                         d_non_corrected=T["no"], bFixScale=False)
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    i = out["info"].cpu().numpy()
    assert i[0] == 0 and i[2] == nkf - 1
    t = float(np.median(ms[1:]))
    scene = "%d key frames, %d + %d + %d + %d edges, %d envelope blocks, %d iterations, %d trials" % (i[1], i[3], i[4], i[5], i[6], i[9], i[7], i[8])
    return ["# Optimizer::OptimizeEssentialGraph on the device, resident call, HIP events around the call alone (its four output arrays are allocated",
            "# inside it), median of 5 after one warm-up: k_eg_prepare, 20 x (k_eg_linearize, k_eg_assemble, k_eg_step), k_eg_finish, of which the",
            "# iterations after the stop flag return at once.  reference = tests/eg_reference.py on the same shape with %d key frames (%d iterations," % (nref, ref["iterations"]),
            "# %d trials), wall clock: OUR dense restatement in numpy on one core, cubic in the key frames, NOT g2o and not a CPU baseline.  No g2o" % ref["trials"],
            "# build exists here to time; no target is set.",
            "%-128s %10s %22s" % ("call", "GPU ms", "reference ms (%d KFs)" % nref),
            "%-128s %10.3f %22.1f" % ("essential_graph: " + scene, t, t_ref)]


def covis_lines(nkf=500, cap=2000, held=1400, npairs=128, conn_cap=256, lkf_cap=256, qcap=16000):
    """The covisibility graph: a whole-map UpdateConnections of a ride-shaped map, its views, and UpdateLocalMap of a batch of frames."""
    rng = np.random.RandomState(11)
    npts = nkf * held // 6
    start = rng.randint(0, nkf, npts)
    length = np.minimum(rng.randint(2, 11, npts), nkf - start)                  # a track: 2..10 consecutive key frames
    obs_start = np.zeros(npts + 1, np.int32)
    obs_start[1:] = np.cumsum(length)
    owner = np.repeat(np.arange(npts), length)
    obs_frame = (np.repeat(start, length) + np.arange(obs_start[-1]) - np.repeat(obs_start[:-1], length)).astype(np.int32)
    kf_point = np.full((nkf + npairs, cap), -1, np.int32)
    n = np.zeros(nkf + npairs, np.int32)
    order = np.argsort(obs_frame, kind="stable")
    for f, lo, hi in zip(range(nkf), np.searchsorted(obs_frame[order], np.arange(nkf)), np.searchsorted(obs_frame[order], np.arange(nkf), "right")):
        pts = owner[order[lo:hi]][:cap]
        kf_point[f, :len(pts)], n[f] = pts, len(pts)
    kp_point = np.full((npairs, cap), -1, np.int32)
    for p_ in range(npairs):                                                    # a frame tracks a share of the points of one key frame
        f = int(rng.randint(0, nkf))
        kp_point[p_, :n[f]:3] = kf_point[f, :n[f]:3]
        n[nkf + p_] = n[f]
    bad = (rng.randint(0, 50, npts) == 0).astype(np.uint8)
    rank = rng.permutation(nkf + npairs).astype(np.int32)
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nfr = nkf + npairs
    T = dict(kf_point=dev(kf_point), n=dev(n), bad=dev(bad), os=dev(obs_start), of=dev(obs_frame), rank=dev(rank), lst=dev(np.arange(nkf, dtype=np.int32)),
             kp=dev(kp_point), pf=dev(np.arange(nkf, nfr, dtype=np.int32)))
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    G = dict(ck=z(nfr, conn_cap), cw=z(nfr, conn_cap), nc=z(nfr), ok=z(nfr, conn_cap), ow=z(nfr, conn_cap), no=z(nfr), par=z(nfr) - 1,
             first=torch.ones(nfr, dtype=torch.uint8, device="cuda"), st=z(nfr), loop=z(64, 3), info=z(4))
    O = dict(best=z(nfr, 10), cs=z(nfr + 1), cv=z(nfr * 64), cvw=z(nfr * 64), bw=z(nfr), vinfo=z(2), kpo=z(npairs, cap), lk=z(npairs, lkf_cap), nl=z(npairs),
             ref=z(npairs), q=z(npairs, qcap), nq=z(npairs), lst=z(npairs))
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, h = ext._L, ext._h

    def update():
        G["nc"].zero_(); G["no"].zero_(); G["par"].fill_(-1); G["first"].fill_(1)
        ext._check(L.pgorb_update_connections_batch_device(h, p(T["kf_point"]), p(T["n"]), nfr, cap, npts, p(T["bad"]), p(T["os"]), p(T["of"]),
                                                           int(obs_start[-1]), p(T["rank"]), None, nkf, p(T["lst"]), 15, conn_cap, p(G["ck"]), p(G["cw"]), p(G["nc"]),
                                                           p(G["ok"]), p(G["ow"]), p(G["no"]), p(G["par"]), p(G["first"]), p(G["st"]), 64, p(G["loop"]), p(G["info"]), s))

    def views():
        ext._check(L.pgorb_covisibility_views_device(h, nfr, conn_cap, p(G["ok"]), p(G["ow"]), p(G["no"]), 10, p(O["best"]), nfr * 64, p(O["cs"]), p(O["cv"]),
                                                     p(O["cvw"]), 30, p(O["bw"]), p(O["vinfo"]), s))

    def local_map():
        ext._check(L.pgorb_update_local_map_batch_device(h, p(T["kf_point"]), p(T["n"]), nfr, cap, None, p(T["pf"]), npairs, p(T["kp"]), npts, p(T["bad"]),
                                                         p(T["os"]), p(T["of"]), int(obs_start[-1]), conn_cap, p(G["ok"]), p(G["no"]), p(G["par"]), p(T["rank"]),
                                                         10, 80, lkf_cap, None, None, p(O["kpo"]), p(O["lk"]), p(O["nl"]), p(O["ref"]), qcap, p(O["q"]), p(O["nq"]),
                                                         p(O["lst"]), s))
    t_up, t_vw, t_lm = timed(update), timed(views), timed(local_map)
    st, nc, no = G["st"].cpu().numpy()[:nkf], G["nc"].cpu().numpy()[:nkf], G["no"].cpu().numpy()[:nkf]
    assert np.all(st & 1) and not np.any(st & 32) and int(O["vinfo"][0]) == 0 and int(G["info"][1]) == 0
    f = nkf // 2                                                               # one row against numpy: the counters of key frame f
    pts = kf_point[f, :n[f]]
    pts = pts[bad[pts] == 0]
    seen = np.concatenate([obs_frame[obs_start[q]:obs_start[q + 1]] for q in pts])
    cnt = np.bincount(seen[seen != f], minlength=nkf)
    row = dict(zip(G["ck"][f, :nc[f]].cpu().numpy().tolist(), G["cw"][f, :nc[f]].cpu().numpy().tolist()))
    assert row == {int(j): int(c) for j, c in enumerate(cnt) if c}, "row %d differs from numpy" % f
    nl, nq, ls = O["nl"].cpu().numpy(), O["nq"].cpu().numpy(), O["lst"].cpu().numpy()
    assert np.all(ls == 0) and nl.min() > 0 and nq.min() > 0
    scene = "%d key frames x %d slots, %d points, %d observations" % (nkf, cap, npts, obs_start[-1])
    return ["# The covisibility graph on the device, resident calls, HIP events, median of 9 after one warm-up.  No CPU baseline exists (the Python",
            "# reference of the tests is not one) and no target is set: this records what was measured.",
            "%-150s %10s" % ("call", "GPU ms"),
            "%-150s %10.3f" % ("update_connections, whole map in list order, th 15: %s; rows hold %.0f counters, %.0f ordered, on average (k_cov_prep, k_cov_count, "
                               "k_cov_finish, k_cov_loop; 4 small resets included)" % (scene, nc.mean(), no.mean()), t_up),
            "%-150s %10.3f" % ("covisibility_views: best 10, the essential graph's CSR (%d entries), GetCovisiblesByWeight(30) lengths" % int(O["vinfo"][1]), t_vw),
            "%-150s %10.3f" % ("update_local_map: %d frames of that map, a third of a key frame's points each: %.0f local key frames, %.0f local points on average"
                               % (npairs, nl.mean(), nq.mean()), t_lm)]


def cull_lines():
    """The cullings: KeyFrameCulling of a ride-shaped map against the Python reference of the tests on one core -- a map with much to cull
    and one with nothing to cull --, MapPointCulling and the compaction of the observation lists."""
    head = ["# The cullings on the device, resident calls, HIP events, median of 9 after one warm-up, the in/out state restored before every call.  The CPU",
            "# column is the literal Python reference of the tests (tests/cull_reference.py) on one core, NOT ORB-SLAM2 and not a tuned baseline.  No target",
            "# is set: this records what was measured.",
            "%-150s %10s %12s" % ("call", "GPU ms", "Python ms")]
    return head + cull_rows(0.5)[:1] + cull_rows(0.55)


def cull_rows(short, nkf=200, cap=2000, conn_cap=256, list_cap=256, nrecent=3000):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cull_cases as K
    import cull_reference as CU
    rng = np.random.RandomState(17)
    w = K.World(nkf, None, [f == 0 for f in range(nkf)])
    for it in range(4 * nkf * cap // 5):                                        # tracks of 2..3 (a share `short` of them) or 4..40 consecutive key frames
        f0 = int(rng.randint(0, nkf))
        ln = int(rng.randint(2, 4)) if rng.rand() < short else int(rng.randint(4, 41))
        fs = [f for f in range(f0, min(f0 + ln, nkf)) if len(w.slots[f]) < cap]
        if len(fs) >= 2:
            w.point(fs, octave={f: int(rng.randint(0, 3)) for f in fs}, ref_kf=fs[int(rng.randint(0, len(fs)))])
        if it % 256 == 0 and min(len(s) for s in w.slots[20:nkf - 20]) >= cap:
            break
    npts, cur = len(w.obs), nkf // 2
    a = K.arrays(w, conn_cap)
    a["conn_kf"][:], a["conn_w"][:], a["ord_kf"][:], a["ord_w"][:] = -1, 0, -1, 0
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    d = K.upload(a)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, h = ext._L, ext._h
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    first, st, info = torch.ones(nkf, dtype=torch.uint8, device="cuda"), z(nkf), z(4)
    ext._check(L.pgorb_update_connections_batch_device(h, p(d["kf_point"]), p(d["n"]), nkf, a["cap"], npts, p(d["point_bad"]), p(d["obs_start"]), p(d["obs_frame"]),
                                                       a["nobs"], None, p(d["id0"]), nkf, p(torch.arange(nkf, dtype=torch.int32, device="cuda")), 15, conn_cap,
                                                       p(d["conn_kf"]), p(d["conn_w"]), p(d["nconn"]), p(d["ord_kf"]), p(d["ord_w"]), p(d["nord"]), p(d["parent"]),
                                                       p(first), p(st), 0, None, p(info), s))
    torch.cuda.synchronize()
    assert not np.any(st.cpu().numpy() & 32)
    inout = ("kf_point", "point_bad", "obs_live", "ref_obs", "kf_bad", "to_be_erased", "conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")
    keep = {k: d[k].clone() for k in inout}
    record, status = z(list_cap, 4), z(nkf)

    def restore():
        for k in inout:
            d[k].copy_(keep[k])

    def cull():
        ext._check(L.pgorb_keyframe_culling_device(h, p(d["kps"]), p(d["kf_point"]), p(d["n"]), nkf, a["cap"], npts, p(d["point_bad"]), p(d["obs_start"]),
                                                   p(d["obs_frame"]), p(d["obs_idx"]), a["nobs"], p(d["obs_live"]), p(d["ref_obs"]), None, p(d["id0"]), None,
                                                   p(d["kf_bad"]), p(d["to_be_erased"]), cur, conn_cap, p(d["conn_kf"]), p(d["conn_w"]), p(d["nconn"]),
                                                   p(d["ord_kf"]), p(d["ord_w"]), p(d["nord"]), p(d["parent"]), list_cap, p(record), p(status), p(info), s))

    def timed_fresh(fn, reps=9):
        ms = []
        for r in range(reps + 1):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:]))
    t_kf = timed_fresh(cull)
    inf = info.cpu().numpy().copy()
    rec = record.cpu().numpy()[:inf[1]]
    assert inf[0] == 0
    # the same map through the Python reference of the tests, one core
    g = {k: keep[k].cpu().numpy() for k in ("conn_kf", "conn_w", "nconn", "ord_kf", "ord_w", "nord", "parent")}
    for f in range(nkf):
        w.conn[f] = {int(j): int(x) for j, x in zip(g["conn_kf"][f, :g["nconn"][f]], g["conn_w"][f, :g["nconn"][f]])}
        w.ordl[f] = [(int(j), int(x)) for j, x in zip(g["ord_kf"][f, :g["nord"][f]], g["ord_w"][f, :g["nord"][f]])]
        w.parent[f] = int(g["parent"][f])
    kfs, pts = K.objects(w)
    t0 = time.perf_counter()
    want = CU.keyframe_culling(kfs[cur], kfs)
    t_ref = (time.perf_counter() - t0) * 1e3
    assert [tuple(int(x) for x in r) for r in rec] == [tuple(r) for r in want], "the device's records differ from the reference's"
    assert np.array_equal(d["kf_bad"].cpu().numpy()[:nkf], np.array([k.bad for k in kfs], np.uint8))
    # MapPointCulling of nrecent points and the compaction, on the state the cull left
    recent = torch.from_numpy(rng.permutation(npts)[:nrecent].astype(np.int32)).cuda()
    nr = int(recent.numel())
    fk, vi, fo = (torch.from_numpy(rng.randint(lo, hi, npts).astype(np.int32)).cuda() for lo, hi in ((96, 101), (1, 40), (0, 12)))
    action, rout, nout, minfo = z(nr), z(nr), z(1), z(4)
    keep2 = {k: d[k].clone() for k in inout}

    def points():
        ext._check(L.pgorb_map_point_culling_device(h, p(d["kf_point"]), p(d["n"]), nkf, a["cap"], npts, p(d["point_bad"]), p(d["obs_start"]), p(d["obs_frame"]),
                                                    p(d["obs_idx"]), a["nobs"], p(d["obs_live"]), p(fk), p(vi), p(fo), nr, p(recent), 100, 2, p(action), p(rout),
                                                    p(nout), p(minfo), s))
    keep = keep2
    t_mp = timed_fresh(points)
    cst, cof, coi, cref, cinfo = z(npts + 1), z(a["nobs"] + 1), z(a["nobs"] + 1), z(npts + 1), z(1)

    def compact():
        ext._check(L.pgorb_compact_observations_device(h, npts, p(d["obs_start"]), p(d["obs_frame"]), p(d["obs_idx"]), a["nobs"], p(d["obs_live"]), p(d["ref_obs"]),
                                                       p(cst), p(cof), p(coi), p(cref), p(cinfo), s))
    t_co = timed(compact)
    assert int(cinfo[0]) == int(d["obs_live"][:a["nobs"]].sum())
    mi = minfo.cpu().numpy()
    scene = "%d key frames x %d slots (%d filled on average), %d points, %d observations" % (nkf, cap, a["n"][:nkf].mean(), npts, a["nobs"])
    return ["%-150s %10.3f %12.1f" % ("keyframe_culling, %.0f%% short tracks: %s; the list of key frame %d has %d members, %d culled, %d points went bad (k_cull_eval, k_cull_walk; "
                                      "2 small resets included)" % (100 * short, scene, cur, inf[1], inf[2], inf[3]), t_kf, t_ref),
            "%-150s %10.3f %12s" % ("map_point_culling: %d recent points of that map, %d survive, %d culled (k_cull_points, one workgroup)" % (nr, mi[1], mi[2]), t_mp, "-"),
            "%-150s %10.3f %12s" % ("compact_observations: %d observations, %d live (k_cull_compact_scan, k_cull_compact_copy)" % (a["nobs"], int(cinfo[0])), t_co, "-")]


def gba_lines(nkf=500, per_kf=40, span=4):
    """GlobalBundleAdjustment: a ride-shaped map in the resident call, and LocalBundleAdjustment's benchmark window through both."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import warnings
    import gba_cases as GC
    import lba_cases as LC
    warnings.simplefilter("ignore")
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)

    def timed(name, reps=5):
        D = GC.device_arrays(GC.case(name)[0])
        ms, r = [], None
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            P, its, robust, in_place = GC.case(name)
            T, cap = D[0], D[1]
            e0.record()
            out = pg.Optimizer.GlobalBundleAdjustment_device(ext, T["kps"], T["n"], cap, T["pose"], len(P.pos), T["pts"], T["os"], T["of"], T["oi"],
                                                             T["pb"], T["kb"], T["id0"], its, robust, in_place)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            r = out["info"].cpu().numpy()
        return float(np.median(ms[1:])), r
    # the ride: points over `span` consecutive key frames, one old loop and the new one
    B, cams = GC._chain(7100, nkf, nkf * per_kf // span, nobs=span, far=20)
    for k in range(40):
        p = B.add_point([B.rng.uniform(-1, 1), B.rng.uniform(-1, 1), B.rng.uniform(25, 35)], 0.3)
        for f in ((3 * nkf // 5, nkf // 10) if k < 20 else (nkf - 2, nkf - 1, 0, 1)):
            B.observe(p, f)
    GC._cache["bench_ride"] = (B.problem([], 0, "bench_ride", extra_keys=0), 10, 0, 0)
    t_ride, i_ride = timed("bench_ride")
    # LBA's benchmark window, through LBA (one workgroup) and through GBA (many) on the same machine in the same run
    W = LC.window("bench", 7000, 20, 20, 2000, nobs=6, noise=0.7, outliers=2000 * 6 // 50, far=20)
    LC._cache["bench"] = (W, 2)
    one = LC.Batch(["bench"])
    r1 = LC.run_gpu_batch(one, ext, time_reps=5)[0]
    li = r1["info"]
    GC._cache["bench_window"] = (W, 10, 0, 0)
    t_win, i_win = timed("bench_window")
    row = lambda i: "%d key frames (%d free), %d points, %d edges, %d envelope blocks, %d iterations, %d trials" % (i[3], i[4], i[2], i[1], i[7], i[5], i[6])
    return ["# Optimizer::GlobalBundleAdjustemnt on the device, resident call, HIP events around the call alone (its six output arrays are allocated",
            "# inside it), median of 5 after one warm-up: k_gba_prepare, 10 x (k_gba_linearize, k_gba_begin, 10 x (k_gba_schur, k_gba_solve, k_gba_try,",
            "# k_gba_decide)), k_gba_finish = 422 launches, of which those behind the stop flag or the end of their iteration return at once.",
            "# The window row is LocalBundleAdjustment's benchmark window; local_ba adjusts its 20 local key frames in one workgroup (two rounds, robust",
            "# first), global_ba all 40 over many workgroups (one round, not robust): compare the time per Levenberg trial.  No g2o build exists",
            "# here to time; no target is set.",
            "%-132s %10s %14s" % ("call", "GPU ms", "GPU ms/trial"),
            "%-132s %10.3f %14.4f" % ("global_ba, ride: " + row(i_ride), t_ride, t_ride / max(int(i_ride[6]), 1)),
            "%-132s %10.3f %14.4f" % ("global_ba, window: " + row(i_win), t_win, t_win / max(int(i_win[6]), 1)),
            "%-132s %10.3f %14.4f" % ("local_ba, window: %d local + %d fixed key frames, %d points, %d edges, %d + %d iterations, %d + %d trials" % (
                li[3], li[4], li[2], li[1], li[5], li[7], li[6], li[8]), one.ms, one.ms / max(int(li[6] + li[8]), 1))]


def loop_correct_lines(nkf=200, cap=2000, nlist=30, fresh=50):
    """Loop correction: both device forms on one ride-shaped map; a sample of the results is held against the Python reference."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import loop_correct_cases as K
    import loop_correct_reference as LR
    rng = np.random.RandomState(29)
    poses = [K.pose(K.rot((0.05, 1, 0.02), 0.9 * f), (0.05 * np.sin(0.3 * f), 0.02 * np.cos(0.2 * f), 4.0 + 0.03 * f)) for f in range(nkf)]
    fill, pts = [0] * nkf, []
    for it in range(4 * nkf * cap // 5):                                        # tracks of 2..40 consecutive key frames
        f0, ln = int(rng.randint(0, nkf)), int(rng.randint(2, 41))
        fs = [f for f in range(f0, min(f0 + ln, nkf)) if fill[f] < cap]
        if len(fs) >= 2:
            for f in fs:
                fill[f] += 1
            pts.append(dict(pos=rng.normal(size=3) * 2.0, holders=fs, ref=fs[int(rng.randint(len(fs)))], octave=int(rng.randint(8))))
        if it % 256 == 0 and min(fill[20:nkf - 20]) >= cap:
            break
    cur = nkf - 1
    lc = K.loop_case("ride", poses, cur, K.sim3_near(poses[cur], 1.1, rng), list(range(cur - nlist, cur)), pts, [int(x) for x in rng.permutation(nkf)])
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    n, nobs = lc["npoints"], len(lc["obs_frame"])

    def timed_fresh(run, D, reps=9):
        keep, ms = D["pts"].clone(), []
        for r in range(reps + 1):
            D["pts"].copy_(keep)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(D, False); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        D["pts"].copy_(keep)
        return float(np.median(ms[1:])), run(D, True)
    D = K.loop_device_arrays(lc)
    t_lc, (got, _) = timed_fresh(lambda D, dl: K.run_device_loop(lc, ext, D=D, download=dl), D)
    t0 = time.perf_counter()
    want = LR.correct_loop(lc)
    t_ref = (time.perf_counter() - t0) * 1e3
    assert K.same(got, want, K.LOOP_KEYS), "the device's correction differs from the reference's: " + K.diff(got, want, K.LOOP_KEYS)
    done = [int(f < nkf - fresh) for f in range(nkf)]
    gba = [K._adjusted(p, rng, 1.0) if done[f] else p for f, p in enumerate(poses)]
    pos = np.array(lc["points"]["pos"], np.float32)
    pdone = [int(done[int(r)] and rng.rand() < 0.9) for r in lc["ref_kf"]]
    mc = K.map_case("ride", poses, gba, done, [-1] + list(range(nkf - 1)), [1] + [0] * (nkf - 1), None, pos, pos + np.float32(0.01), pdone, None, lc["ref_kf"])
    M = K.map_device_arrays(mc)
    t_mu, (gotm, _) = timed_fresh(lambda M, dl: K.run_device_map(mc, ext, D=M, download=dl), M)
    t0 = time.perf_counter()
    wantm = LR.update_map(mc)
    t_refm = (time.perf_counter() - t0) * 1e3
    assert K.same(gotm, wantm, K.MAP_KEYS), "the device's map update differs from the reference's: " + K.diff(gotm, wantm, K.MAP_KEYS)
    scene = "%d key frames x %d slots (%d filled on average), %d points, %d observations" % (nkf, cap, np.mean(fill), n, nobs)
    li, mi = got["info"], gotm["info"]
    return ["# Loop correction on the device, resident calls, HIP events around the call alone, median of 9 after one warm-up, the",
            "# table restored before every call.  The Python column is the literal reference of the tests (tests/loop_correct_reference.py) on one core, whose",
            "# bytes the GPU's must equal; it is NOT ORB-SLAM2 and not a tuned baseline.  The parent commit has no such path and ORB-SLAM2 cannot be built",
            "# here, so there is nothing measured to compare against: no target is set and no time is a pass condition.",
            "%-150s %10s %12s" % ("call", "GPU ms", "Python ms"),
            "%-150s %10.3f %12.1f" % ("correct_loop_poses: %s; %d members, %d points corrected (k_lc_init, k_lc_rank, k_lc_members, k_lc_claim, k_lc_points)" % (
                scene, li[1], li[2]), t_lc, t_ref),
            "%-150s %10.3f %12.1f" % ("global_ba_map_update: the same map, the last %d key frames not adjusted (a chain); %d key frames updated, %d recomputed, %d points "
                                      "updated (k_mu_kf, k_mu_points)" % (fresh, mi[1], mi[2], mi[3]), t_mu, t_refm)]


def trajectory_lines():
    """The trajectory read-out: predict + commit over 8 and 128 trackers, the same hand-off done on the host, and GetTrajectory of an
    hour's records; the results are held against the numpy reference of the tests."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_pose_cases as K
    import track_pose_reference as TR
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    L, h, q = ext._L, ext._h, K._q
    s = torch.cuda.current_stream()
    sp = C.c_void_p(s.cuda_stream)

    def events(run, reps=9, inner=50):
        # the calls take tens of microseconds: an event pair spans `inner` back-to-back calls and the row reports the time per call
        ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                run()
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        return float(np.median(ms[1:]))
    ref = K.run_sequences_reference()
    state, frames = K.track_sequences()
    fr, x, cap = frames[3], frames[3]["trackers"], 4096
    rows = []
    for ntrack in (8, 128):
        rep = ntrack // 2
        S0 = K._up(ref[2]["state"]).repeat(rep)
        T = torch.zeros(ntrack * cap * 72, dtype=torch.uint8, device="cuda")
        T.view(ntrack, cap * 72)[:, :K.CAP * 72] = K._up(ref[2]["traj"]).view(2, K.CAP * 72).repeat(rep, 1)
        N0 = K._up(ref[2]["count"]).repeat(rep)
        S, N = S0.clone(), N0.clone()
        kf, modes = K._up(fr["kf"]), K._up(np.array([v["mode"] for v in x], np.int32)).repeat(rep)
        pred, ps, cs = K._sent(ntrack * 84), K._sent(ntrack * 4), K._sent(ntrack * 4)
        ok, rk = K._up(np.array([v["ok"] for v in x], np.uint8)).repeat(rep), K._up(np.array([v["ref_kf"] for v in x], np.int32)).repeat(rep)
        tm, ids = K._up(np.array([v["time"] for v in x], np.float64)).repeat(rep), K._up(np.array([v["id"] for v in x], np.int64)).repeat(rep)

        def device():
            S.copy_(S0); N.copy_(N0)
            assert L.pgorb_track_predict_batch_device(h, ntrack, 0, q(modes), q(S), q(T), cap, q(N), 4, q(kf), q(pred), q(ps), sp) == 0
            # the predicted pose stands in for PoseOptimization's result: commit reads it where predict left it
            assert L.pgorb_track_commit_batch_device(h, ntrack, q(S), q(pred), q(ok), q(rk), q(tm), q(ids), 4, q(kf), q(T), cap, q(N), q(cs), sp) == 0
        t_dev = events(device)
        assert torch.equal(pred, K._up(ref[3]["pred"]).repeat(rep)) and int(N.view(torch.int32).min()) == int(N.view(torch.int32).max()) == 4, "predict / commit differ from the reference"

        kf_h = fr["kf"]

        def host():
            # the old way: download the last pose and record, form the products in numpy, upload the prediction; after the
            # optimisation download its pose, form velocity and record on the host, upload
            st = np.frombuffer(S0.cpu().numpy().tobytes(), K.TRACK_STATE_DTYPE).copy()
            rec = np.frombuffer(T.view(ntrack, cap * 72)[:, 2 * 72:3 * 72].contiguous().cpu().numpy().tobytes(), K.TRAJECTORY_RECORD_DTYPE)
            out = np.zeros(ntrack, K.KF_POSE_DTYPE)
            for t in range(ntrack):
                trk = TR.Tracker(st[t], [rec[t]])
                out[t], _ = TR.predict(trk, int(x[t % 2]["mode"]), kf_h)
                st[t] = trk.state()
            d = K._up(out)
            back = np.frombuffer(d.cpu().numpy().tobytes(), K.KF_POSE_DTYPE)
            for t in range(ntrack):
                trk = TR.Tracker(st[t], [rec[t]])
                TR.commit(trk, back[t], x[t % 2]["ok"], x[t % 2]["ref_kf"], x[t % 2]["time"], x[t % 2]["id"], kf_h, cap)
                st[t] = trk.state()
            K._up(st)
        t0 = time.perf_counter()
        host()
        t_host = (time.perf_counter() - t0) * 1e3
        rows.append("%-150s %10.4f %12.2f" % ("track_predict + track_commit, %d trackers, resident (k_tp_predict, k_tp_commit) | the same hand-off through the "
                                              "host: 2 downloads, numpy products, 2 uploads" % ntrack, t_dev, t_host))
    w = K.random_world(1, 108000, 2000, culled=0.3, exact=True)
    t0 = time.perf_counter()
    want = TR.get_trajectory_batched(w)
    t_ref = (time.perf_counter() - t0) * 1e3
    D, n = K.table_device_arrays(w), len(w["traj"])
    traj = K._up(w["traj"])
    O = dict(quat_wxyz=K._sent(n * 32), translation=K._sent(n * 24), time_usec=K._sent(n * 8), frame_id=K._sent(n * 8), is_lost=K._sent(n), status=K._sent(n * 4),
             info=K._sent(16))

    def read_out():
        assert L.pgorb_get_trajectory_device(h, 2000, q(D["pose"]), q(D["bad"]), q(D["par"]), q(D["ids"]), q(D["tcp"]), n, q(traj), None, q(O["quat_wxyz"]),
                                             q(O["translation"]), q(O["time_usec"]), q(O["frame_id"]), q(O["is_lost"]), q(O["status"]), q(O["info"]), sp) == 0
    t_traj = events(read_out)
    assert K.same(K.download_trajectory(O, n), want), "the device's trajectory differs from the reference's"
    depth = max(TR.chain_depth(w, i) for i in range(0, n, 97))
    rows.append("%-150s %10.4f %12.2f" % ("get_trajectory: %d records over 2000 key frames, %d culled, chains up to %d deep in a sample; %d lost (k_traj_origin, "
                                          "k_traj_records) | the batched numpy reference" % (n, int(w["kf_bad"].sum()), depth, int(want["is_lost"].sum())), t_traj, t_ref))
    return ["# The trajectory read-out on the device (csrc/track_pose.hip), resident calls, HIP events around 50 back-to-back calls, time per call, median of 9",
            "# after one warm-up (predict + commit: the two launches and the reset of the state and the count in front of them).",
            "# The second column is the same work on the host in numpy on one core (the restatement of the tests, whose bytes the GPU's must equal), wall",
            "# clock, one run, transfers included where the row says so; it is NOT ORB-SLAM2 and not a tuned baseline.  The parent commit has no such path, so",
            "# there is nothing measured to compare against: no target is set and no time is a pass condition.",
            "%-150s %10s %12s" % ("call", "GPU ms", "host ms")] + rows


def edit_lines():
    """The map edits: three list shapes through pgorb_apply_map_edits_device, next to the host replay of tests/map_edit_reference.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_edit_cases as K
    import map_edit_reference as R
    import time
    rng = np.random.RandomState(23)
    nkf, nslots, npts = 24, 1200, 4000
    free = [list(rng.permutation(nslots - 1)) for _ in range(nkf)]              # the last slot of every key frame stays free
    lists = []
    for p in range(npts):
        f0, ln = int(rng.randint(0, nkf - 1)), int(rng.randint(2, 7))
        lists.append([(f, int(free[f].pop())) for f in range(f0, min(f0 + ln, nkf - 1))])        # nobody sees the last key frame yet
    a = K.world(nkf, nslots, lists, list(rng.permutation(nkf)))
    new = nkf - 1
    shapes = []
    adds = rng.choice(npts, 500, replace=False)
    shapes.append(("500 independent ADDs (a new key frame: ProcessNewKeyFrame)", K.E(*[(R.ADD, int(p), new, i) for i, p in enumerate(adds)])))
    rows, used = [], set()
    for k in range(200):                                                        # Fuse-shaped: ADDED / MERGED / REPLACED over pairs of points, NOP in between
        x, y = (int(v) for v in rng.choice(npts, 2, replace=False))
        u = rng.rand()
        rows.append((R.NOP, 0, 0, 0) if u < 0.3 or x in used or y in used else (R.ADD, x, new, 600 + k, ) if u < 0.55 else (R.REPLACE, x, y, 0))
        used.update((x, y))
    shapes.append(("a Fuse-shaped list of 200 mixed edits (ADD, REPLACE, NOP)", K.E(*rows)))
    star = rng.choice(npts, 201, replace=False)
    shapes.append(("200 REPLACEs into one survivor (one component, one wave)", K.E(*[(R.REPLACE, int(p), int(star[0]), 0) for p in star[1:]])))
    ext = pg.ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    out = []
    for name, edits in shapes:
        c = K.Case(name, a, edits)
        t0 = time.perf_counter()
        e = K.expected(c, exact=False)
        t_ref = (time.perf_counter() - t0) * 1e3
        d = K.upload(c, e)
        keep = {k: d[k].clone() for k in ("kf_point", "point_bad", "visible", "found", "replaced")}
        ms = []
        for rep in range(10):
            for k, v in keep.items():
                d[k].copy_(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); K.run_device(c, ext, e, d=d); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        got = K.download(d)
        assert K.same(got, e), ("the device's result differs from the reference's", name, K.diff(got, e))
        out.append("%-150s %10.4f %12.2f" % ("apply_map_edits: %s; %d points, %d observations, %d components, %d slot writes" %
                                             (name, npts, a["nobs"], int(e["info"][4]), int(e["info"][5])), float(np.median(ms[1:])), t_ref))
    return ["# The map edits on the device (csrc/map_edit.hip), resident calls, HIP events around one call (seven launches and two memsets), median of 9 after one",
            "# warm-up, the in/out state restored before every call.  The second column is the host replay of the same list by the literal Python objects of the",
            "# tests (tests/map_edit_reference.py; building the objects from the arrays and back included) on one core, wall clock, one run; NOT ORB-SLAM2 and not a tuned baseline.  The parent commit has no device",
            "# form, so there is nothing measured to compare against: NEITHER NUMBER IS A TARGET and no time is a pass condition.",
            "%-150s %10s %12s" % ("call", "GPU ms", "Python ms")] + out


if a.edit_only:
    lines = ["# python tools/next_tier_bench.py --edit-only   (MI355X)"] + edit_lines()
    print("\n".join(lines))
    open(a.out or os.path.join(ROOT, "profiles", "next_tier_map_edit.txt"), "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.trajectory_only:
    lines = ["# python tools/next_tier_bench.py --trajectory-only   (MI355X)"] + trajectory_lines()
    print("\n".join(lines))
    open(a.out or os.path.join(ROOT, "profiles", "next_tier_trajectory.txt"), "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.loop_correct_only:
    lines = ["# python tools/next_tier_bench.py --loop-correct-only   (MI355X)"] + loop_correct_lines()
    print("\n".join(lines))
    open(a.out or os.path.join(ROOT, "profiles", "next_tier_loop_correct.txt"), "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.cull_only:
    lines = ["# python tools/next_tier_bench.py --cull-only   (MI355X)"] + cull_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.gba_only:
    lines = ["# python tools/next_tier_bench.py --gba-only   (MI355X)"] + gba_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.eg_only:
    lines = ["# python tools/next_tier_bench.py --eg-only   (MI355X)"] + eg_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.lba_only:
    lines = ["# python tools/next_tier_bench.py --lba-only   (MI355X)"] + lba_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.optsim3_only:
    lines = ["# python tools/next_tier_bench.py --optsim3-only   (MI355X)"] + optsim3_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.pnp_only:
    lines = ["# python tools/next_tier_bench.py --pnp-only   (MI355X)"] + pnp_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.sim3_only:
    lines = ["# python tools/next_tier_bench.py --sim3-only   (MI355X)"] + sim3_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.pose_only:
    lines = ["# python tools/next_tier_bench.py --pose-only   (MI355X)"] + pose_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.covis_only:
    lines = ["# python tools/next_tier_bench.py --covis-only   (MI355X)"] + covis_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.track_only:
    lines = ["# python tools/next_tier_bench.py --track-only   (MI355X)"] + track_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.loop_only:
    lines = ["# python tools/next_tier_bench.py --loop-only   (MI355X)"] + loop_lines()
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.place_only:
    lines = ["# python tools/next_tier_bench.py --place-only   (MI355X)"] + place_lines(pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
if a.refresh_only:
    lines = ["# python tools/next_tier_bench.py --refresh-only   (MI355X)"] + refresh_lines(refresh_rows(pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)))
    print("\n".join(lines))
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    sys.exit(0)
ride = synth_ride(0, w, h, B)
ext = pg.ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
fr = torch.from_numpy(ride).cuda()
p = lambda t: C.c_void_p(t.data_ptr())
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)


rows = []
t_plain = timed(lambda: ext.extract_batch_device(fr))
rgb = fr.flip(2).unsqueeze(-1).expand(B, h, w, 3).contiguous()          # grey value in all channels, mirrored: ingest undoes it
t_ing = timed(lambda: ext.extract_batch_ingest_device(rgb, True, 0, False, True))
k2, d2, n2 = ext.extract_batch_ingest_device(rgb, True, 0, False, True)
kps, desc, n = ext.extract_batch_device(fr)
ext.check_async(); torch.cuda.synchronize()
assert torch.equal(n, n2) and all(torch.equal(d2[f, :n[f]], desc[f, :n[f]]) and torch.equal(k2[f, :n[f]].view(torch.int32), kps[f, :n[f]].view(torch.int32)) for f in range(B))   # (4899 + 9617 + 1868) v + 8192 >> 14 == v
kps, desc, n = kps.clone(), desc.clone(), n.clone()
cap = kps.shape[1]
nh = n.cpu().numpy()
r0 = rgb[0].cpu().numpy()
orb_oracle.ingest_geometry(orb_oracle.rgb_to_gray(r0), 0, False, True)          # (first call loads the library)
t0 = time.time(); g = orb_oracle.ingest_geometry(orb_oracle.rgb_to_gray(r0), 0, False, True); c_ing = (time.time() - t0) * B * 1e3
assert np.array_equal(g, ride[0])
rows.append(("ingest (RGB->grey + hflip), beyond plain extraction", t_ing - t_plain, 3 * w * h * B, c_ing))

cam = (C.c_float * 4)(1400.0, 1400.0, 960.0, 540.0); dist = (C.c_float * 5)(-0.28, 0.07, 0.0002, 0.00002, 0.0)
und = torch.empty_like(kps)
t_und = timed(lambda: ext._check(ext._L.pgorb_undistort_keypoints_batch_device(ext._h, p(kps), p(n), B, cap, cam, dist, p(und), s)))
kh = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
k0 = kh[0, :nh[0]].copy().view(orb_oracle.KEYPOINT_DTYPE).reshape(-1)
t0 = time.time(); orb_oracle.undistort_keypoints(k0, list(cam), list(dist)); c_und = (time.time() - t0) * B * 1e3
rows.append(("undistort keypoints", t_und, int(nh.sum()) * 56, c_und))

gs = torch.empty((B, 3073), dtype=torch.int32, device="cuda"); gi = torch.empty((B, cap), dtype=torch.int32, device="cuda")
t_grid = timed(lambda: ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(kps), p(n), B, cap, 0.0, float(w), 0.0, float(h), p(gs), p(gi), s)))
t0 = time.time(); orb_oracle.frame_grid(k0, (0.0, float(w), 0.0, float(h))); c_grid = (time.time() - t0) * B * 1e3
rows.append(("frame grid 64x48", t_grid, int(nh.sum()) * 28 + B * 3073 * 4, c_grid))

f1 = torch.arange(0, B - 1, dtype=torch.int32, device="cuda"); f2 = torch.arange(1, B, dtype=torch.int32, device="cuda")
prev0 = kps[:B - 1, :, :2].contiguous()
prev = prev0.clone(); m12 = torch.empty((B - 1, cap), dtype=torch.int32, device="cuda"); nm = torch.empty(B - 1, dtype=torch.int32, device="cuda")
def init_match():
    prev.copy_(prev0)
    ext._check(ext._L.pgorb_search_for_initialization_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(f1), p(f2), B - 1,
               0.0, float(w), 0.0, float(h), p(prev), p(m12), p(nm), 100, C.c_float(0.9), 1, s))
t_copy = timed(lambda: prev.copy_(prev0))
t_sfi = timed(init_match) - t_copy
dh = desc.cpu().numpy()
k1 = kh[1, :nh[1]].copy().view(orb_oracle.KEYPOINT_DTYPE).reshape(-1)
t0 = time.time()
onm, _, _ = orb_oracle.search_for_initialization(k0, dh[0, :nh[0]], k1, dh[1, :nh[1]], (0.0, float(w), 0.0, float(h)), np.stack([k0["x"], k0["y"]], 1))
c_sfi = (time.time() - t0) * (B - 1) * 1e3
assert int(nm[0]) == onm
rows.append(("SearchForInitialization (%d pairs, %d matches/pair)" % (B - 1, int(nm.float().mean())), t_sfi, int(nh.sum()) * (28 + 32) * 2, c_sfi))

dsc, wgt, par = V.synth_vocabulary_fast(10, 6, seed=7)
voc = V.ORBVocabulary(blob=V.pack_vocabulary(10, 6, dsc, wgt, par))
voc.upload(ext)
flat = torch.cat([desc[f, :nh[f]] for f in range(B)]).contiguous()
nd = flat.shape[0]
word = torch.empty(nd, dtype=torch.int32, device="cuda"); wt = torch.empty(nd, dtype=torch.float64, device="cuda"); node = torch.empty(nd, dtype=torch.int32, device="cuda")
t_bow = timed(lambda: ext._check(ext._L.pgorb_bow_transform_device(ext._h, p(flat), nd, 4, p(word), p(wt), p(node), s)))
rows.append(("BoW transform, k=10 L=6 (%d descriptors)" % nd, t_bow, nd * (32 + 6 * 10 * 32), float("nan")))

# ---- the SLAM-state matchers (a11): single host calls (H2D + kernel + D2H, wall clock), median of 9, one frame pair ----------
def wall(fn, reps=9):
    fn(); ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


F1, F2 = pg.Frame(ext, ride[0]), pg.Frame(ext, ride[1])
rng = np.random.RandomState(5)
nk = F1.N
sel = np.concatenate([rng.permutation(nk)[: int(nk * 0.8)]] * 1)
px = (F1.mvKeys["x"][sel] - 2 + rng.uniform(-1.5, 1.5, len(sel))).astype(np.float32)       # the ride moves (2, 1) px per frame
py = (F1.mvKeys["y"][sel] - 1 + rng.uniform(-1.5, 1.5, len(sel))).astype(np.float32)
valid = (rng.uniform(size=len(sel)) > 0.05).astype(np.uint8); obs = (rng.uniform(size=len(sel)) > 0.1).astype(np.uint8)
lvl = F1.mvKeys["octave"][sel].astype(np.int32); vc = np.full(len(sel), 0.9995, np.float32); pdsc = F1.mDescriptors[sel]
mp = pg.MapPoints(valid, px, py, lvl, vc, pdsc, obs)
sf = ext.GetScaleFactors()
host_rows = []
m = pg.ORBmatcher(0.8, True)
g_ms = wall(lambda: m.SearchByProjection(F2, mp, 3.0, None))
t0 = time.perf_counter(); onm, _ = orb_oracle.search_by_projection_points(F2.mvKeys, F2.mDescriptors, F2.bounds, sf, None, valid, px, py, lvl, vc, pdsc, obs, 3.0, 0.8); c_ms = (time.perf_counter() - t0) * 1e3
host_rows.append(("SearchByProjection(Frame, MapPoints, th 3), %d points -> %d" % (len(sel), onm), g_ms, c_ms))
m = pg.ORBmatcher(0.9, True)
ang = F1.mvKeys["angle"][sel].copy()
g_ms = wall(lambda: m.SearchByProjectionLastFrame(F2, valid, px, py, lvl, ang, pdsc, obs, 15.0))
t0 = time.perf_counter(); onm, _ = orb_oracle.search_by_projection_frame(F2.mvKeys, F2.mDescriptors, F2.bounds, sf, None, valid, px, py, lvl, ang, pdsc, obs, 15.0, True); c_ms = (time.perf_counter() - t0) * 1e3
host_rows.append(("SearchByProjection(Frame, LastFrame, th 15), %d points -> %d" % (len(sel), onm), g_ms, c_ms))
_, fvK = voc.transform(F1.mDescriptors, 4); _, fvF = voc.transform(F2.mDescriptors, 4)
kvalid = (rng.uniform(size=F1.N) > 0.3).astype(np.uint8)
m = pg.ORBmatcher(0.7, True)
g_ms = wall(lambda: m.SearchByBoW(ext, F1.mDescriptors, F1.mvKeys["angle"], kvalid, fvK, F2, fvF))
t0 = time.perf_counter(); onm, _ = orb_oracle.search_by_bow(F1.mDescriptors, F1.mvKeys["angle"], kvalid, fvK, F2.mDescriptors, F2.mvKeys["angle"], fvF, 0.7, True); c_ms = (time.perf_counter() - t0) * 1e3
host_rows.append(("SearchByBoW(KeyFrame, Frame), %d nodes -> %d" % (len(fvK[0]), onm), g_ms, c_ms))
sm = pg.ORBmatcher(0.9, True)
prevm = np.stack([F1.mvKeys["x"], F1.mvKeys["y"]], 1).astype(np.float32)
g_ms = wall(lambda: sm.SearchForInitialization(F1, F2, prevm.copy(), 100))
host_rows.append(("SearchForInitialization(F1, F2, 100), one pair through the host API", g_ms, c_sfi / (B - 1)))


def sideways_geometry(frames_apart, focal=500.0):
    """F12 and the epipole of a sideways motion along the ride's (2, 1) px shift (LocalMapping::ComputeF12, float32)."""
    K = np.array([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]], np.float32)
    Ki = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    t = np.array([0.02 * frames_apart, 0.01 * frames_apart, 1e-4], np.float32)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float32)
    return (Ki.T @ tx @ Ki).astype(np.float32), (np.float32(focal * t[0] / t[2] + w / 2.0), np.float32(focal * t[1] / t[2] + h / 2.0))


F12h, eph = sideways_geometry(1)
has1 = (rng.uniform(size=F1.N) < 0.3).astype(np.uint8); has2 = (rng.uniform(size=F2.N) < 0.3).astype(np.uint8)
m = pg.ORBmatcher(0.6, True)
tnm, _ = m.SearchForTriangulation(F1, F2, F12h, eph, fvK, fvF, has1, has2)
g_ms = wall(lambda: m.SearchForTriangulation(F1, F2, F12h, eph, fvK, fvF, has1, has2))
host_rows.append(("SearchForTriangulation(KF1, KF2, F12), %d nodes -> %d" % (len(fvK[0]), tnm), g_ms, float("nan")))

# ---- round 3: the same three matchers as BATCHED, RESIDENT calls: every frame against its predecessor, all pairs in one launch ----
npairs = B - 1
qn = min(int(nk * 0.8), 2000)
qcap = qn
def rep(a, dt):                                      # the same query set for every pair (frame f's keypoints projected into f + 1)
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(a[:qn], dt), (npairs,) + np.asarray(a[:qn]).shape))).cuda()
qsel = []
vq, xq, yq, lq, cq, aq, dq, oq = [], [], [], [], [], [], [], []
for f in range(npairs):
    kf = kh[f, :nh[f]].copy().view(orb_oracle.KEYPOINT_DTYPE).reshape(-1)
    ss = rng.permutation(nh[f])[:qn]
    m = len(ss)
    pad = lambda a, dt: np.concatenate([np.asarray(a, dt), np.zeros((qcap - m,) + np.asarray(a).shape[1:], dt)])
    vq.append(pad((rng.uniform(size=m) > 0.05), np.uint8)); xq.append(pad(kf["x"][ss] - 2 + rng.uniform(-1.5, 1.5, m), np.float32))
    yq.append(pad(kf["y"][ss] - 1 + rng.uniform(-1.5, 1.5, m), np.float32)); lq.append(pad(kf["octave"][ss], np.int32))
    cq.append(pad(np.full(m, 0.9995), np.float32)); aq.append(pad(kf["angle"][ss], np.float32)); dq.append(pad(dh[f, ss], np.uint8))
    oq.append(pad((rng.uniform(size=m) > 0.1), np.uint8)); qsel.append(m)
T = lambda L_: torch.from_numpy(np.stack(L_)).cuda()
vq, xq, yq, lq, cq, aq, dq, oq = T(vq), T(xq), T(yq), T(lq), T(cq), T(aq), T(dq), T(oq)
nqd = torch.tensor(qsel, dtype=torch.int32, device="cuda")
pairF = torch.arange(1, B, dtype=torch.int32, device="cuda"); pairK = torch.arange(0, B - 1, dtype=torch.int32, device="cuda")
asg = torch.empty((npairs, cap), dtype=torch.int32, device="cuda"); nmb = torch.empty(npairs, dtype=torch.int32, device="cuda")
bnd = (0.0, float(w), 0.0, float(h))
batch_rows = []
t_pp = timed(lambda: ext._check(ext._L.pgorb_search_by_projection_points_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(pairF), npairs, *bnd,
             None, qcap, p(nqd), p(vq), p(xq), p(yq), p(lq), p(cq), p(dq), p(oq), 3.0, 0.8, p(asg), p(nmb), s)))
batch_rows.append(("SearchByProjection(Frame, MapPoints, th 3): %d pairs x %d points -> %d" % (npairs, qn, int(nmb.float().mean())), t_pp, host_rows[0][2]))
t_pf = timed(lambda: ext._check(ext._L.pgorb_search_by_projection_frame_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(gs), p(gi), p(pairF), npairs, *bnd,
             None, qcap, p(nqd), p(vq), p(xq), p(yq), p(lq), p(aq), p(dq), p(oq), 15.0, 1, p(asg), p(nmb), s)))
batch_rows.append(("SearchByProjection(Frame, LastFrame, th 15): %d pairs x %d points -> %d" % (npairs, qn, int(nmb.float().mean())), t_pf, host_rows[1][2]))
wordb = torch.empty((B, cap), dtype=torch.int32, device="cuda"); wtb = torch.empty((B, cap), dtype=torch.float64, device="cuda"); nodeb = torch.empty((B, cap), dtype=torch.int32, device="cuda")
ext._check(ext._L.pgorb_bow_transform_device(ext._h, p(desc), B * cap, 4, p(wordb), p(wtb), p(nodeb), s))
fvn = torch.empty((B, cap), dtype=torch.int32, device="cuda"); fvs = torch.empty((B, cap + 1), dtype=torch.int32, device="cuda")
fvf = torch.empty((B, cap), dtype=torch.int32, device="cuda"); nfvd = torch.empty(B, dtype=torch.int32, device="cuda")
t_fv = timed(lambda: ext._check(ext._L.pgorb_feature_vectors_batch_device(ext._h, p(nodeb), p(n), B, cap, p(fvn), p(fvs), p(fvf), p(nfvd), s)))
batch_rows.append(("FeatureVector of %d frames (CSR by node, on the device)" % B, t_fv, float("nan")))
kfvd = torch.from_numpy((rng.uniform(size=(npairs, cap)) > 0.3).astype(np.uint8)).cuda()
t_bw = timed(lambda: ext._check(ext._L.pgorb_search_by_bow_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfvd), p(pairK), p(pairF), npairs,
             p(kfvd), 0.7, 1, p(asg), p(nmb), s)))
batch_rows.append(("SearchByBoW(KeyFrame, Frame): %d pairs -> %d" % (npairs, int(nmb.float().mean())), t_bw, host_rows[2][2]))
# SearchForTriangulation: every 5th frame from the 21st on is a new key frame matched against its 20 predecessors (CreateNewMapPoints'
# covisible neighbours), all pairs in one launch; the per-pair figures divide by these pairs, not by npairs
tri = [(k, k - d) for k in range(20, B, 5) for d in range(1, 21)]
ntri = len(tri)
if ntri:
    geo = [sideways_geometry(a - b) for a, b in tri]
    tF = torch.from_numpy(np.stack([g[0].reshape(9) for g in geo])).cuda()
    tE = torch.from_numpy(np.array([g[1] for g in geo], np.float32)).cuda()
    tA = torch.tensor([a for a, _ in tri], dtype=torch.int32, device="cuda"); tB = torch.tensor([b for _, b in tri], dtype=torch.int32, device="cuda")
    tH1 = torch.from_numpy((rng.uniform(size=(ntri, cap)) < 0.3).astype(np.uint8)).cuda()
    tH2 = torch.from_numpy((rng.uniform(size=(ntri, cap)) < 0.3).astype(np.uint8)).cuda()
    tM = torch.empty((ntri, cap), dtype=torch.int32, device="cuda"); tN = torch.empty(ntri, dtype=torch.int32, device="cuda")
    t_tr = timed(lambda: ext._check(ext._L.pgorb_search_for_triangulation_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfvd),
                 p(tA), p(tB), ntri, p(tF), p(tE), p(tH1), p(tH2), 1, p(tM), p(tN), s)))
    batch_rows.append(("SearchForTriangulation: %d key frames x 20 neighbours = %d pairs -> %d" % (ntri // 20, ntri, int(tN.float().mean())),
                       t_tr, float("nan"), ntri))
    # CreateNewMapPoints (LocalMapping.cc:209-454) for the same key frames and neighbours in one call: the ride is a sideways camera over
    # a fronto-parallel plane at depth 1 (frame k at (2k/f, k/f, 0), R = I), so matches triangulate; 30 % of the keypoints have a point
    kfs = list(range(20, B, 5))
    poses = np.zeros(B, pg.KF_POSE_DTYPE)
    for k in range(B):
        poses[k] = pg.kf_pose(np.hstack([np.eye(3), [[-2.0 * k / 500.0], [-1.0 * k / 500.0], [0.0]]]), (2.0 * k / 500.0, 1.0 * k / 500.0, 0.0),
                              500.0, 500.0, w / 2.0, h / 2.0)
    cP = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    cH = torch.from_numpy((rng.uniform(size=(B, cap)) < 0.3).astype(np.uint8)).cuda()
    cK = torch.tensor(kfs, dtype=torch.int32, device="cuda")
    cN = torch.tensor([[k - d for d in range(1, 21)] for k in kfs], dtype=torch.int32, device="cuda")
    cNN = torch.full((len(kfs),), 20, dtype=torch.int32, device="cuda"); cMD = torch.ones((len(kfs), 20), dtype=torch.float32, device="cuda")
    cPts = torch.empty((len(kfs), cap * pg.NEW_MAP_POINT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    cNP = torch.empty(len(kfs), dtype=torch.int32, device="cuda"); cC = torch.empty((len(kfs), 20), dtype=torch.int32, device="cuda")
    cHo = torch.empty((len(kfs), cap), dtype=torch.uint8, device="cuda")
    t_cnm = timed(lambda: ext._check(ext._L.pgorb_create_new_map_points_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(fvn), p(fvs), p(fvf), p(nfvd),
                  p(cP), p(cH), p(cK), len(kfs), p(cN), p(cNN), 20, p(cMD), p(cPts), p(cNP), p(cC), None, None, p(cHo), s)))
    batch_rows.append(("CreateNewMapPoints: %d key frames x 20 neighbours = %d pairs -> %d points / key frame" % (len(kfs), 20 * len(kfs), int(cNP.float().mean())),
                       t_cnm, float("nan"), 20 * len(kfs)))
    # ... one key frame through the host API, and the matcher-only host path it replaces: 20 single SearchForTriangulation calls
    kf0 = kfs[-1]
    KFs = {k: pg.Frame(ext, ride[k]) for k in [kf0] + [kf0 - d for d in range(1, 21)]}
    fvh = {k: voc.transform(F.mDescriptors, 4)[1] for k, F in KFs.items()}
    hh = {k: (rng.uniform(size=F.N) < 0.3).astype(np.uint8) for k, F in KFs.items()}
    nb = [kf0 - d for d in range(1, 21)]
    g_cnm = wall(lambda: pg.LocalMapping.CreateNewMapPoints(KFs[kf0], [KFs[k] for k in nb], fvh[kf0], [fvh[k] for k in nb], poses[kf0],
                                                            [poses[k] for k in nb], np.ones(20, np.float32), hh[kf0], [hh[k] for k in nb]))
    m = pg.ORBmatcher(0.6, False)
    geoh = {k: sideways_geometry(kf0 - k) for k in nb}
    g_loop = wall(lambda: [m.SearchForTriangulation(KFs[kf0], KFs[k], *geoh[k], fvh[kf0], fvh[k], hh[kf0], hh[k]) for k in nb])
    host_rows.append(("CreateNewMapPoints(KF, 20 neighbours), one key frame", g_cnm, float("nan")))
    host_rows.append(("20 x SearchForTriangulation, one key frame (matcher only; no triangulation)", g_loop, float("nan")))

    # Fuse (ORBmatcher.cc:827-979) as SearchInNeighbors calls it (LocalMapping.cc:491): the key frame's points fused into each target.
    # Map points are keypoints lifted onto the ride's plane at depth 1 (frame k's camera at (2k/f, k/f, 0)); every frame's slots hold
    # a point for 30 % of its keypoints; one shared table
    fuse_ids = np.arange(B, dtype=np.uint64) + 1000
    kh, dh = kps.cpu().numpy().view(pg.KEYPOINT_DTYPE).reshape(B, cap), desc.cpu().numpy().reshape(B, cap, 32)
    sfh = ext.GetScaleFactors()

    def lift(f, idx):
        k = kh[f, idx]
        pt = np.zeros(len(idx), pg.MAP_POINT_DTYPE)
        pt["pos"][:, 0] = (k["x"] - w / 2.0) / 500.0 + 2.0 * f / 500.0
        pt["pos"][:, 1] = (k["y"] - h / 2.0) / 500.0 + 1.0 * f / 500.0
        pt["pos"][:, 2] = 1.0
        pt["normal"][:, 2] = 1.0
        pt["max_distance"] = np.float32(np.sqrt(1 + ((k["x"] - w / 2.0) / 500.0) ** 2 + ((k["y"] - h / 2.0) / 500.0) ** 2)) * sfh[k["octave"]]
        pt["min_distance"] = pt["max_distance"] / sfh[7]
        return pt, dh[f, idx]
    tp, td, tobs, qidx, slot = [], [], [], {}, np.full((B, cap), -1, np.int32)
    base = 0
    for f in range(B):
        idx = np.nonzero(rng.uniform(size=int(nh[f])) < 0.3)[0]
        pt, dd = lift(f, idx)
        tp.append(pt); td.append(dd); tobs.append(np.full(len(idx), fuse_ids[f]))
        slot[f, idx] = base + np.arange(len(idx)); base += len(idx)
    for k in kfs:                                                      # the key frame's new points (not yet in any slot)
        idx = np.arange(min(int(nh[k]), 1500))
        pt, dd = lift(k, idx)
        tp.append(pt); td.append(dd); tobs.append(np.full(len(idx), fuse_ids[k]))
        qidx[k] = base + idx; base += len(idx)
    tP, tD, tO = np.concatenate(tp), np.concatenate(td), np.concatenate(tobs).astype(np.uint64)
    tS = np.arange(len(tP) + 1, dtype=np.int32)
    # one call through the host API: key frame kf0's 1500 points into its predecessor, with a table of the points that call reads
    tgt = kf0 - 1
    Ft = KFs[tgt]
    own = slot[tgt, :Ft.N]
    used = np.concatenate([own[own >= 0], qidx[kf0]])
    remap = np.full(len(tP), -1, np.int32); remap[used] = np.arange(len(used))
    small = pg.MapPointTable(tP[used], tD[used], None, np.arange(len(used) + 1, dtype=np.int32), tO[used])
    s_own, s_q = np.where(own >= 0, remap[np.maximum(own, 0)], -1).astype(np.int32), remap[qidx[kf0]]
    g_fuse = wall(lambda: pg.ORBmatcher().Fuse(Ft, poses[tgt], int(fuse_ids[tgt]), s_own, small, s_q, 3.0))
    nfz = pg.ORBmatcher().Fuse(Ft, poses[tgt], int(fuse_ids[tgt]), s_own, small, s_q, 3.0)[0]
    # the sequential reference's matching step on the same inputs (tests/fuse_reference.py, Python), for scale
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fuse_reference as FR
    import matcher_cases as MCs
    inv_s2 = np.array([np.float32(1.0) / np.float32(x * x) for x in sfh], np.float32)
    rkf = FR.KeyFrame(int(fuse_ids[tgt]), Ft.mvKeysUndistorted, Ft.mDescriptors, poses[tgt], (0.0, float(w), 0.0, float(h)), sfh, inv_s2,
                      np.float32(FR._LOG_F()(sfh[1])), 8)
    rmp = [FR.MapPoint(i, tP[i]["pos"], tP[i]["normal"], tP[i]["min_distance"], tP[i]["max_distance"], tD[i]) for i in qidx[kf0]]
    t0 = time.perf_counter(); [FR.match(rkf, mp_) for mp_ in rmp]; c_fuse = (time.perf_counter() - t0) * 1e3
    host_rows.append(("Fuse(KF, %d points, th 3) -> %d fused, one call" % (len(qidx[kf0]), nfz), g_fuse, c_fuse))
    # batched: every key frame's points into its 20 predecessors, 22 x 20 independent problems in one call
    probs = [(k, k - d) for k in kfs for d in range(1, 21)]
    qcap = 1500
    Q = np.full((len(probs), qcap), -1, np.int32); NQ = np.zeros(len(probs), np.int32)
    for i, (k, t) in enumerate(probs):
        Q[i, :len(qidx[k])] = qidx[k]; NQ[i] = len(qidx[k])
    G = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    zgs = torch.empty((B, 3073), dtype=torch.int32, device="cuda"); zgi = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_frame_grid_batch_device(ext._h, p(kps), p(n), B, cap, 0.0, float(w), 0.0, float(h), p(zgs), p(zgi), s))
    zK, zId, zSl = G(np.array([t for _, t in probs], np.int32)), G(fuse_ids.view(np.int64)), G(slot)
    zP, zD, zS, zO, zQ, zN = G(tP.view(np.uint8)), G(tD), G(tS), G(tO.view(np.int64)), G(Q), G(NQ)
    zA = torch.empty((len(probs), qcap), dtype=torch.int32, device="cuda"); zNF = torch.empty(len(probs), dtype=torch.int32, device="cuda")
    zSo = torch.empty((len(probs), cap), dtype=torch.int32, device="cuda")
    t_fz = timed(lambda: ext._check(ext._L.pgorb_fuse_batch_device(ext._h, p(kps), p(desc), p(n), cap, p(zgs), p(zgi), p(zK), len(probs), p(zId), p(cP),
                 0.0, float(w), 0.0, float(h), p(zSl), len(tP), p(zP), p(zD), None, p(zS), p(zO), qcap, p(zN), p(zQ), 3.0, p(zA), None, None,
                 p(zSo), p(zNF), s)))
    batch_rows.append(("Fuse: %d key frames x 20 targets = %d problems x %d points -> %d fused" % (len(kfs), len(probs), qcap, int(zNF.float().mean())),
                       t_fz, c_fuse, len(probs)))

lines = ["# python tools/next_tier_bench.py --batch %d --features %d   (MI355X; ms per %d-frame 1080p batch; CPU = oracle, 1 thread, one frame or pair scaled to the batch)" % (B, nf, B),
         "# extraction alone (K1-K6): %.3f ms" % t_plain,
         "%-58s %10s %12s %12s %10s" % ("kernel", "GPU ms", "us / frame", "GB/s (alg.)", "CPU ms")]
for name, ms, byts, cpu in rows:
    lines.append("%-58s %10.3f %12.2f %12.1f %10.0f" % (name, ms, ms * 1e3 / B, byts / ms / 1e6, cpu))
lines.append("# single host calls on one 1080p frame pair (upload + kernel + download, wall clock ms) next to the oracle's")
lines.append("%-72s %10s %10s" % ("call", "GPU ms", "CPU ms"))
for name, g, cc in host_rows:
    lines.append("%-72s %10.3f %10.2f" % (name, g, cc))
lines.append("# round 3: batched, resident forms (every frame vs its predecessor, one launch for all pairs; GPU ms per batch and per pair) next to the oracle's one-core ms per pair")
lines.append("%-86s %10s %12s %12s" % ("call", "GPU ms", "GPU ms/pair", "CPU ms/pair"))
for name, g, cc, *np_ in batch_rows:
    lines.append("%-86s %10.3f %12.4f %12.2f" % (name, g, g / (np_[0] if np_ else npairs), cc))
lines += refresh_lines(refresh_rows(ext))
lines += track_lines()
print("\n".join(lines))
if a.out:
    open(a.out, "w").write("\n".join(lines) + "\n")
