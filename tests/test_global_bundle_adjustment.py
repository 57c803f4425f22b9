"""pgorb_global_bundle_adjustment (pilotguru_amd/csrc/global_ba.hip): Optimizer::GlobalBundleAdjustemnt on the GPU against the plain
reference of tests/gba_reference.py on the constructed maps of tests/gba_cases.py.

The CPU tests check presence, the C++ mirror, the set derivation against a literal transcription of Optimizer.cc:71-184, what each
rule mutant changes, the case condition under every arithmetic form, the reference's optimum against scipy.optimize.least_squares,
and keep tests/golden/gba_spread.json up to date.  The GPU tests compare the single call and the device form with the reference
(integers, flags and statuses exactly, floats by gba_cases.bounds = max(2 float ulps, 16 x the recorded spread of the reference's own
forms)), the single call with the device form byte for byte, the device form on a second stream, repeated and after a problem of
another size has used the arena, the chain into pgorb_refresh_map_points_batch_device, the refusals and the envelope limit.

On the MI355X every integer and every float output of every case equalled the reference's bit for bit (the recorded spread between
the reference's forms is 0 in every float output, so the bound is 2 float ulps).  The map update after the adjustment
(LoopClosing.cc:679-742) is not built and has no test here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import gba_cases as GC  # noqa: E402
import gba_reference as GR  # noqa: E402
import lba_cases as LC  # noqa: E402
import map_point_reference as MR  # noqa: E402
import pose_reference as PR  # noqa: E402

f32, f64 = np.float32, np.float64
NAMES = ("pgorb_global_bundle_adjustment", "pgorb_global_bundle_adjustment_device")
SUITE_FORMS = {n: [GR.Form()] for n in GC.ONE_FORM}          # the other cases run under all twelve


# ---------------------------------------------------------------- presence
def test_symbols_and_mirrors_are_present():
    """The two entry points are exported and refuse a NULL context; both mirrors and the constants exist and agree with the header."""
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    z = np.zeros(64, f32)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_global_bundle_adjustment(None, 0, p, p, p, None, None, 0, p, None, p, p, p, 10, 0, 0, p, p, p, p, None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_global_bundle_adjustment_device(None, p, p, 0, 1, p, None, None, 0, p, None, p, p, p, 0, 10, 0, 0, p, p, p, p, None, p,
                                                   None) == _lib.PGORB_E_ARG
    assert (pg.GBA_NOTHING, pg.GBA_NONFINITE, pg.GBA_LIMIT, pg.GBA_INFO) == (GR.GBA_NOTHING, GR.GBA_NONFINITE, GR.GBA_LIMIT, GR.INFO)
    assert (pg.GBA_MAX_KF, pg.GBA_MAX_POINTS, pg.GBA_MAX_EDGES, pg.GBA_MAX_ENVELOPE_BLOCKS) == (GR.MAX_KF, GR.MAX_POINTS, GR.MAX_EDGES,
                                                                                               GR.MAX_ENVELOPE_BLOCKS)
    assert callable(pg.Optimizer.GlobalBundleAdjustment) and callable(pg.Optimizer.GlobalBundleAdjustment_device)
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "GlobalBundleAdjustmentResult GlobalBundleAdjustment(" in hpp and "pgorb_global_bundle_adjustment(ctx_" in hpp
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    assert all(("int  %s(" % n) in hdr for n in NAMES)
    for text in ("#define PGORB_GBA_INFO           8", "#define PGORB_GBA_MAX_KF         2048", "#define PGORB_GBA_MAX_POINTS     262144",
                 "#define PGORB_GBA_MAX_EDGES      2097152", "#define PGORB_GBA_MAX_ENVELOPE_BLOCKS 131072", "#define PGORB_GBA_LIMIT          4"):
        assert text in hdr, text


def test_cpp_mirror_compiles():
    """host/orb_extractor.hpp with the new mirror is valid C++17 (syntax only: no device is needed)."""
    src = ("#include \"orb_extractor.hpp\"\nint main() { pgorb::Optimizer o(nullptr); std::vector<pgorb_map_point> pts; "
           "pgorb::MapPointObservations obs; obs.obsStart.push_back(0);\n"
           "auto r = o.GlobalBundleAdjustment({}, {}, {}, pts, {}, obs, 10, false, true); return r.optimised; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "pilotguru_amd", "host"), "-x", "c++", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


def test_huber_delta_is_the_float_of_sqrt_5_99():
    assert GR.DELTA == f64(f32(2.4474475)) and GR.DELTA != PR.DELTA
    src = open(os.path.join(ROOT, "pilotguru_amd", "csrc", "global_ba.hip")).read()
    assert float(f32(GR.DELTA)).hex().replace("0000000p", "p") + "f" in src


# ---------------------------------------------------------------- the derivation and the cases
def test_set_derivation_equals_the_literal_transcription():
    for n in GC.CASE_NAMES:
        P = GC.case(n)[0]
        vertex, edge, included = GR.derive_sets(P)
        vs, fixed, edges, marked = GR.literal_sets(P)
        pt_of = np.repeat(np.arange(len(P.pos)), np.diff(P.obs_start))
        assert set(np.flatnonzero(vertex)) == vs, n
        assert set((int(pt_of[k]), int(P.obs_frame[k])) for k in np.flatnonzero(edge)) == edges, n
        assert set(np.flatnonzero(included)) == marked, n
        assert fixed == set(int(f) for f in np.flatnonzero(P.fixed_id0) if not P.kf_bad[f]), n
        r = GC.run_reference(n)
        assert set(np.flatnonzero(r["point_done"])) == marked and set(np.flatnonzero(r["kf_done"])) == vs, n


def test_cases_hold_what_they_claim():
    r = {n: GC.run_reference(n) for n in GC.CASE_NAMES}
    P = {n: GC.case(n)[0] for n in GC.CASE_NAMES}
    assert list(r["init2"]["info"][[3, 4, 7]]) == [2, 1, 1] and GC.case("init2")[1:] == (20, 0, 1)
    assert r["init2"]["info"][6] > r["init2"]["info"][5], "init2 has rejected trials"
    assert r["chain5"]["info"][3] == 5 and r["chain5"]["info"][7] < 4 * 5 // 2 + 4                # a band, not the full triangle
    assert r["ring24"]["info"][3] == 24 and r["ring24"]["info"][7] > 23 * 3                       # the closing points fill the skyline
    assert GC.case("robust")[2] == 1
    b, Pb = r["bad"], P["bad"]
    lens = np.diff(Pb.obs_start)
    pt_of = np.repeat(np.arange(len(Pb.pos)), lens)
    assert Pb.kf_bad.sum() >= 2 and Pb.point_bad.sum() >= 1
    only_bad = [p for p in range(len(Pb.pos)) if lens[p] and not Pb.point_bad[p] and Pb.kf_bad[Pb.obs_frame[pt_of == p]].all()]
    assert only_bad and not b["point_done"][only_bad].any()
    lone = [f for f in range(Pb.nframes) if not Pb.kf_bad[f] and not (Pb.obs_frame == f).any()]
    assert lone and b["kf_done"][lone].all() and not b["pose_is_input"][lone].any()
    assert not P["no_gauge"].fixed_id0.any() and r["no_gauge"]["info"][4] == r["no_gauge"]["info"][3]
    assert r["nothing"]["info"][0] == GR.GBA_NOTHING and r["nothing"]["info"][1] == 0
    assert r["nonfinite"]["info"][0] == GR.GBA_NONFINITE and np.isfinite(P["nonfinite"].pos).all()
    w, Pw = r["wide"], P["wide"]
    assert Pw.nframes == 70 and len(Pw.pos) > 2560 and np.bincount(Pw.obs_frame).max() > 1024 and np.diff(Pw.obs_start).max() == 40
    assert w["info"][0] == 0 and w["info"][4] > 64
    assert r["envelope_limit"]["info"][0] == GR.GBA_LIMIT and r["envelope_limit"]["info"][7] == 513 * 514 // 2 > GR.MAX_ENVELOPE_BLOCKS


def test_spread_file_is_up_to_date():
    """tests/golden/gba_spread.json (tests/golden/make_gba_spread.py writes it) holds what the reference shows now; the cases of
    gba_cases.ONE_FORM are recorded there once and not measured again here."""
    rec = GC.recorded_spread()
    assert sorted(rec) == sorted(GC.CASE_NAMES)
    for n in GC.CASE_NAMES:
        if n in GC.ONE_FORM:
            continue
        now = GC.spread(n)
        assert sorted(now) == sorted(rec[n]), n
        for k in now:
            assert abs(now[k] - rec[n][k]) <= 1e-3 * max(now[k], rec[n][k]) + 1e-300, (n, k, now[k], rec[n][k])


def test_every_case_meets_the_case_condition_under_every_form():
    """No Levenberg decision near its threshold and the same integers under all twelve arithmetic forms (one form for the cases of
    gba_cases.ONE_FORM): the reference alone shows that the exact comparisons are safe."""
    rec = GC.recorded_spread()
    bad = [b for n in GC.CASE_NAMES for b in GC.condition(n, rec[n], SUITE_FORMS.get(n))]
    assert bad == [], bad[:5]


def _as_got(P, r):
    poses = LC.pose_records(P)
    out = poses.copy()
    for f in range(P.nframes):
        if not r["pose_is_input"][f]:
            out["Tcw"][f], out["Ow"][f] = r["pose_Tcw"][f].reshape(out["Tcw"][f].shape), r["pose_Ow"][f]
    return dict(r, camera_kept=True, pose_bytes=[out[f].tobytes() for f in range(P.nframes)], pose_in_bytes=[poses[f].tobytes() for f in range(P.nframes)])


def _changed(rules, names):
    rec = GC.recorded_spread()
    return [n for n in names if GC.differences(GC.case(n)[0], GC.run_reference(n), _as_got(GC.case(n)[0], GC.run_reference(n, rules=rules)), rec[n])]


def test_every_mutant_changes_a_compared_output():
    small = [n for n in GC.CASE_NAMES if n not in GC.ONE_FORM]
    assert _changed(GR.REFERENCE, small) == []
    for m, rules in GR.MUTANTS.items():
        assert _changed(rules, small), m
    assert "robust" in _changed(GR.MUTANTS["delta_5991"], ["robust"])
    assert "bad" in _changed(GR.MUTANTS["no_round_trip_for_unmoved_key_frames"], ["bad"])
    assert "bad" in _changed(GR.MUTANTS["points_without_edges_marked"], ["bad"])
    assert "bad" in _changed(GR.MUTANTS["bad_kf_observations_kept"], ["bad"])
    assert "chain5" in _changed(GR.MUTANTS["id0_not_fixed"], ["chain5"])


@pytest.mark.parametrize("name", GC.ANCHORED)
def test_reference_reaches_the_optimum_scipy_finds(name):
    """An independent anchor: scipy.optimize.least_squares on the same residuals from the same start.  The bound is 16 x the relative
    difference measured when tests/golden/gba_spread.json was written (it depends on where each method stops)."""
    rec = GC.recorded()["anchor"][name]
    chi_ref, chi_sp, rel = GC.anchor(name)
    print("%s: reference %.12g, scipy %.12g, relative difference %.3g (recorded %.3g, bound %.3g)" % (name, chi_ref, chi_sp, rel,
                                                                                                  rec["relative_difference"], rec["bound"]))
    assert rec["bound"] == 16.0 * rec["relative_difference"]
    assert rel <= rec["bound"]


def test_mirror_refuses_malformed_input_without_a_device():
    """Optimizer.GlobalBundleAdjustment raises ValueError for what the library's checked call refuses, before the library is called."""
    class Ext:
        def GetLevels(self):
            return LC.NLEVELS
    P = GC.case("chain5")[0]
    for what, kw in _malformed(P):
        with pytest.raises(ValueError):
            _mirror(P, Ext(), **kw)
            pytest.fail(what)


def _mirror(P, ext, **kw):
    import pilotguru_amd as pg
    a = dict(key_frames=GC.frames_of(P, ext), poses=LC.pose_records(P), points=LC.table(P), obs_start=P.obs_start, obs_frame=P.obs_frame.copy(),
             obs_idx=P.obs_idx.copy(), iterations=10, ext=ext)
    a.update(kw)
    return pg.Optimizer.GlobalBundleAdjustment(**a)


def _malformed(P):
    bad_pose, bad_fx, bad_pts = LC.pose_records(P), LC.pose_records(P), LC.table(P)
    bad_pose["Tcw"][1, 3] = np.nan
    bad_fx["fx"][0] = 0.0
    bad_pts["pos"][2, 1] = np.inf
    twice, far, nokf = P.obs_frame.copy(), P.obs_idx.copy(), P.obs_frame.copy()
    twice[1] = twice[0]
    far[0] = 10 ** 6
    nokf[0] = P.nframes
    return (("iterations", dict(iterations=-1)), ("pose", dict(poses=bad_pose)), ("fx", dict(poses=bad_fx)), ("point", dict(points=bad_pts)),
            ("start", dict(obs_start=P.obs_start[::-1].copy())), ("twice", dict(obs_frame=twice)), ("idx", dict(obs_idx=far)),
            ("frame", dict(obs_frame=nokf)))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, LC.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=4)
    assert np.array_equal(np.asarray(e.GetInverseScaleSigmaSquares(), f32)[:LC.NLEVELS], LC.INV_SIGMA2)
    yield e
    e.close()


def _check(name, want, got, what):
    P, _, _, in_place = GC.case(name)
    rec = GC.recorded_spread()[name]
    d = GC.scaled_differences(P, want, got)
    print("%s (%s): " % (name, what) + ", ".join("%s %.2g / %.2g" % (k, d[k], GC.bounds(rec)[k]) for k in GC.FLOAT_OUTPUTS))
    assert GC.differences(P, want, got, rec) == [], "%s (%s)" % (name, what)
    start = np.asarray(LC.table(P))
    assert LC.other_bytes(got["table"]) == LC.other_bytes(start), "%s: normal and distances keep their bytes" % name
    notdone = np.flatnonzero(got["point_done"] == 0)
    assert got["pos"][notdone].tobytes() == P.pos[notdone].tobytes(), "%s: only included points move" % name
    if in_place and not want["info"][0]:
        assert got["table"]["pos"].tobytes() == got["pos"].tobytes(), "%s: in_place writes pos_out into the table" % name
    else:
        assert got["table"].tobytes() == start.tobytes(), "%s: the table is not written" % name


@pytest.fixture(scope="module")
def devices(ext):
    return {n: GC.run_gpu_device(n, ext)[0] for n in GC.CASE_NAMES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", GC.CASE_NAMES)
def test_gpu_device_form_equals_the_reference(ext, devices, name):
    _check(name, GC.run_reference(name), devices[name], "device")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in GC.CASE_NAMES if n != "envelope_limit"])
def test_gpu_single_call_equals_the_reference_and_the_device_form_byte_for_byte(ext, devices, name):
    got = GC.run_gpu(name, ext)
    _check(name, GC.run_reference(name), got, "single")
    assert got["ret"] == GC.run_reference(name)["ret"]
    assert got["all_bytes"] == devices[name]["all_bytes"], name


@pytest.mark.gpu
def test_gpu_envelope_limit_is_a_status_of_the_device_form_and_an_error_of_the_single_call(ext, devices):
    from pilotguru_amd import _lib
    got = devices["envelope_limit"]
    assert got["info"][0] == GR.GBA_LIMIT and got["info"][7] == 513 * 514 // 2 and not got["chi2"].any() and got["kf_done"].all()
    with pytest.raises(_lib.PgorbError) as e:
        GC.run_gpu("envelope_limit", ext)
    assert e.value.code == _lib.PGORB_E_LIMIT


@pytest.mark.gpu
def test_gpu_result_is_the_same_on_a_second_stream_repeated_and_after_another_problem_used_the_arena(ext, devices):
    import torch
    for n in ("ring24", "robust", "bad"):
        assert GC.run_gpu_device(n, ext, torch.cuda.Stream())[0]["all_bytes"] == devices[n]["all_bytes"], (n, "second stream")
        GC.run_gpu_device("wide" if n == "ring24" else "init2", ext)                     # another size in the same arena
        assert GC.run_gpu_device(n, ext)[0]["all_bytes"] == devices[n]["all_bytes"], (n, "after another problem")
        assert GC.run_gpu_device(n, ext)[0]["all_bytes"] == devices[n]["all_bytes"], (n, "repeated")


@pytest.mark.gpu
def test_gpu_chain_into_the_map_point_refresh_on_resident_arrays(ext):
    """GBA with in_place -> pgorb_refresh_map_points_batch_device (normal and depth, select = the done points) with nothing downloaded
    in between, against SetWorldPos followed by UpdateNormalAndDepth (tests/map_point_reference.py)."""
    import torch
    from pilotguru_amd.orb import MAP_POINT_DTYPE, MP_NORMAL_DEPTH
    name = "init2"
    P = GC.case(name)[0]
    D = GC.device_arrays(P)
    r, D, out = GC.run_gpu_device(name, ext, D=D)
    T, cap = D[0], D[1]
    nf, npts, nobs = P.nframes, len(P.pos), len(P.obs_frame)
    sel = torch.nonzero(out["point_done"]).to(torch.int32).reshape(-1).contiguous()
    status = torch.zeros(max(int(sel.numel()), 1), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((nf, cap, 32), dtype=torch.uint8, device="cuda")
    d_pd = torch.zeros((npts, 32), dtype=torch.uint8, device="cuda")
    d_ref = torch.zeros(npts, dtype=torch.int32, device="cuda")
    q = lambda t: C.c_void_p(t.data_ptr())
    ext._check(ext._L.pgorb_refresh_map_points_batch_device(
        ext._h, q(T["kps"]), q(d_desc), q(T["n"]), nf, cap, q(out["pose_out"]), q(T["kb"]), npts, q(T["pts"]), q(d_pd), q(T["pb"]), q(T["os"]),
        q(T["of"]), q(T["oi"]), nobs, q(d_ref), int(sel.numel()), q(sel), MP_NORMAL_DEPTH, None, q(status),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    rows = np.frombuffer(T["pts"].cpu().numpy().tobytes(), MAP_POINT_DTYPE)
    _check(name, GC.run_reference(name), r, "chain")
    sf = np.asarray(ext.GetScaleFactors(), f32)
    kfs = [MR.KeyFrame(LC.keypoints(P.keys_xy[f], P.octaves[f]), np.zeros((len(P.octaves[f]), 32), np.uint8), r["pose_Ow"][f]) for f in range(nf)]
    assert r["point_done"].any()
    for p in np.flatnonzero(r["point_done"]):
        mp = MR.MapPoint(r["pos"][p], np.zeros(32, np.uint8))
        mp.obs = [(kfs[P.obs_frame[k]], int(P.obs_idx[k])) for k in range(P.obs_start[p], P.obs_start[p + 1])]
        mp.ref = mp.obs[0][0]
        assert MR.update_normal_and_depth(mp, sf, LC.NLEVELS)
        assert rows["pos"][p].tobytes() == r["pos"][p].tobytes()
        assert rows["normal"][p].tobytes() == mp.normal.tobytes() and f32(rows["min_distance"][p]) == mp.min_d and \
            f32(rows["max_distance"][p]) == mp.max_d, p


@pytest.mark.gpu
def test_gpu_library_refuses_malformed_input(ext):
    """The checked call refuses on the host; what the Python mirror would stop first goes through the C ABI."""
    from pilotguru_amd import _lib
    from pilotguru_amd.orb import KF_POSE_DTYPE
    L, h = ext._L, ext._h
    P = GC.case("chain5")[0]

    def call(nkf=None, npoints=None, iterations=10, null=(), **kw):
        nf, npts, nobs = P.nframes, len(P.pos), len(P.obs_frame)
        ks = [LC.keypoints(P.keys_xy[f], P.octaves[f]) for f in range(nf)]
        for f, i, o in kw.get("octave", ()):
            ks[f]["octave"][i] = o
        kps = (C.c_void_p * nf)()
        for f in range(nf):
            kps[f] = ks[f].ctypes.data
        a = dict(n=np.array([len(o) for o in P.octaves], np.int32), pose=LC.pose_records(P), pts=LC.table(P), os=P.obs_start.copy(),
                 of=P.obs_frame.copy(), oi=P.obs_idx.copy())
        a.update({k: v for k, v in kw.items() if k in a})
        out = dict(po=np.zeros(nf, KF_POSE_DTYPE), pos=np.zeros((npts, 3), f32), kd=np.zeros(nf, np.uint8), pd=np.zeros(npts, np.uint8),
                   chi=np.zeros(nobs, f32), info=np.zeros(GR.INFO, np.int32))
        p = lambda k, arr: None if k in null else arr.ctypes.data_as(C.c_void_p)
        return L.pgorb_global_bundle_adjustment(h, nf if nkf is None else nkf, kps, p("n", a["n"]), p("pose", a["pose"]), None,
                                                P.fixed_id0.ctypes.data_as(C.c_void_p),
                                                npts if npoints is None else npoints, p("pts", a["pts"]), None, p("os", a["os"]), p("of", a["of"]),
                                                p("oi", a["oi"]), iterations, 0, 0, p("po", out["po"]), p("pos", out["pos"]), p("kd", out["kd"]),
                                                p("pd", out["pd"]), p("chi", out["chi"]), p("info", out["info"]))
    assert call() == GC.run_reference("chain5")["ret"]
    bad_pose, bad_fx, bad_pts = LC.pose_records(P), LC.pose_records(P), LC.table(P)
    bad_pose["Tcw"][1, 3] = np.nan
    bad_fx["fy"][0] = 0.0
    bad_pts["pos"][2, 1] = np.inf
    twice, far, nokf, start0, down = P.obs_frame.copy(), P.obs_idx.copy(), P.obs_frame.copy(), P.obs_start.copy(), P.obs_start.copy()
    twice[1] = twice[0]
    far[0] = 10 ** 6
    nokf[0] = -1
    start0[0] = 1
    down[3] = down[2] - 1
    nneg = np.array([len(o) for o in P.octaves], np.int32)
    nneg[1] = -1
    f0, i0 = int(P.obs_frame[0]), int(P.obs_idx[0])
    for what, kw in (("nkf", dict(nkf=-1)), ("npoints", dict(npoints=-1)), ("iterations", dict(iterations=-1)), ("null pose", dict(null=("pose",))),
                     ("null obs_start", dict(null=("os",))), ("null pose_out", dict(null=("po",))), ("null pos_out", dict(null=("pos",))),
                     ("null obs_frame", dict(null=("of",))), ("n", dict(n=nneg)), ("pose", dict(pose=bad_pose)), ("fy", dict(pose=bad_fx)),
                     ("point", dict(pts=bad_pts)), ("start0", dict(os=start0)), ("down", dict(os=down)), ("twice", dict(of=twice)),
                     ("idx", dict(oi=far)), ("frame", dict(of=nokf)), ("octave", dict(octave=[(f0, i0, LC.NLEVELS)])),
                     ("octave below", dict(octave=[(f0, i0, -1)]))):
        assert call(**kw) == _lib.PGORB_E_ARG, what
    # the capacities, from the counts alone
    assert call(nkf=GR.MAX_KF + 1) == _lib.PGORB_E_LIMIT and call(npoints=GR.MAX_POINTS + 1) == _lib.PGORB_E_LIMIT
    assert call() == GC.run_reference("chain5")["ret"], "the context still works after the refusals"
