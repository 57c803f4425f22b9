"""Every entry point at its stated capacity and one past it (tests/capacity_cases.py).

On the CPU: every case's wanted result (from the family's sequential reference) holds the last valid index of each field it
fills and an index with the field's top bit set, and a field one bit too narrow would change it.  On the GPU: the single call
and the *_batch_device form give the reference's result at capacity, bit for bit, and answer PGORB_E_LIMIT one past it."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the table at the end)
import capacity_cases as CC  # noqa: E402
import matcher_cases as MC  # noqa: E402
import matcher_reference as R  # noqa: E402

_WANT = {}
REFERENCE_SECONDS = {}          # case name -> wall seconds of the sequential reference (profiles/capacity_tests.txt)


def wanted(cc, run=MC.run_reference):
    """The reference's result of a capacity case, computed once per session."""
    if cc["name"] not in _WANT:
        t0 = time.perf_counter()
        _WANT[cc["name"]] = run(cc["case"])
        REFERENCE_SECONDS[cc["name"]] = time.perf_counter() - t0
    return _WANT[cc["name"]]


def check_fields(cc, want):
    """The wanted result reaches the end of every field, uses its top bit, and would change under a narrower field."""
    for fname, f in cc["fields"].items():
        used = sorted(set(int(i) for i in f["used"](want)))
        limit, h = f["limit"], CC.half(f["limit"])
        assert used and used[-1] == limit - 1, "%s: %s never holds the last valid index %d (max %s)" % (cc["name"], fname, limit - 1, used[-1:])
        assert any(i & h for i in used), "%s: %s never has bit %d set" % (cc["name"], fname, h.bit_length() - 1)
        assert all(0 <= i < limit for i in used)
        assert CC.truncated(used, limit) != used, "%s: %s survives a field one bit narrower" % (cc["name"], fname)
        for low, high in f["ties"]:
            assert high % h == low and high in used and low not in used, \
                "%s: %s rivals (%d, %d): the wanted result must hold the high one only" % (cc["name"], fname, low, high)
            assert low in CC.truncated([high], limit)


# ---------------------------------------------------------------- CPU
def _place_many_reference(cc):
    t, rows = cc["case"], cc["query_rows"]
    per = {r: t.reference(r) for r in sorted(set(rows))}
    return dict(per=per, ncand=np.array([len(per[r]["cand"]) for r in rows], np.int32))


@functools.lru_cache(maxsize=None)
def families():
    """(family, cases, reference) of every family but the extractor and K7, which the C oracle answers."""
    import fuse_cases as FC
    import loop_cases as LC
    import mapping_cases as MP
    import triangulation_cases as TC
    return [("grid+sfi", [CC.grid_capacity_case(), CC.sfi_capacity_case()], MC.run_reference),
            ("sbp", CC.sbp_capacity_cases(), MC.run_reference),
            ("bow", [CC.bow_capacity_case()], MC.run_reference),
            ("kfbow", [CC.kfbow_capacity_case()], LC.run_ref1),
            ("tri", [CC.tri_capacity_case()], TC.run_reference),
            ("fuse", [CC.fuse_capacity_case()], FC.run_reference),
            ("ps3", CC.ps3_capacity_cases(), LC.run_ref3),
            ("fs3", [CC.fs3_capacity_case()], LC.run_ref4),
            ("sim3", [CC.sim3_capacity_case()], LC.run_ref2),
            ("cnm", [CC.cnm_capacity_case()], lambda c: MP.run_reference(*c)),
            ("place", [CC.place_capacity_case("reloc"), CC.place_capacity_case("loop")], lambda t: t.reference(0)),
            ("place_queries", [CC.place_many_queries_case("reloc")], None)]


def _all_cases():
    out = []
    for fam, cases, ref in families():
        for cc in cases:
            out.append(pytest.param(cc, ref, id=cc["name"]))
    return out


def want_of(cc, ref):
    if ref is None:
        return wanted(dict(cc, case=cc), _place_many_reference)
    return wanted(cc, ref)


@pytest.mark.parametrize("cc,ref", _all_cases())
def test_cases_fill_their_fields(cc, ref):
    check_fields(cc, want_of(cc, ref))


def test_sbp_points_lie_on_the_lds_line():
    """Each (keypoints, queries) point fits the budget and one more query does not; 16 000 keypoints do not fit even alone."""
    for cap, qcap in CC.SBP_POINTS:
        assert CC.sbp_lds(cap, qcap) <= CC.LDS < CC.sbp_lds(cap, qcap + 1)
    assert CC.SBP_POINTS[0] == (12582, 1) and CC.sbp_lds(12583, 1) > CC.LDS
    assert CC.sbp_lds(CC.KP_MAX, 0) > CC.LDS


def test_cnm_last_neighbour_is_first_to_triangulate():
    """The 64th neighbour creates points of its own: for those keypoints no earlier slot triangulated."""
    fam = [f for f in families() if f[0] == "cnm"][0]
    cc = fam[1][0]
    pts, count = want_of(cc, fam[2])[:2]
    assert len(cc["case"][1]) == CC.CNM_NEIGH and sum(1 for p in pts if p[0] == CC.CNM_NEIGH - 1) > 0
    assert int(count[CC.CNM_NEIGH - 1]) > 0 and {-1, 0} <= set(int(x) for x in count)      # skipped and empty slots in between


def test_ps3_dense_case_overflows_the_list_and_names_the_last_keypoint():
    """More than 64 keypoints within TH_LOW of the first query's descriptor in its window (k_ps3_decide evaluates that query in
    place), the keypoint in the last slot among them; the last slot is taken."""
    import loop_cases as LC
    cc = [c for _, cs, _ in families() for c in cs if c["name"].startswith("ps3_dense")][0]
    c = cc["case"]
    q = int.from_bytes(c.points[c.queries[0]]["desc"].tobytes(), "little")
    live = np.flatnonzero(c.kf[1]["octave"] == 0)
    d = {int(i): bin(int.from_bytes(c.kf[2][i].tobytes(), "little") ^ q).count("1") for i in live}
    assert len(live) == 80 and sum(x <= 50 for x in d.values()) > 64 and d[CC.KP_MAX - 1] <= 50
    assert want_of(cc, LC.run_ref3)[1][CC.KP_MAX - 1] >= 0


def test_k7_case_fills_the_train_index(oracle):
    cc = CC.k7_capacity_case()
    check_fields(cc, wanted(dict(cc, case=cc), lambda c: oracle.hamming_best2(c["a"], c["b"])))


def extractor_want(case, oracle):
    return wanted(dict(case, case=case), lambda c: oracle.OrbOracle(c["nfeatures"], 1.2, c["nlevels"], 20, 7).extract(c["img"]))


@pytest.mark.parametrize("case", CC.extractor_capacity_cases(), ids=lambda c: c["name"])
def test_extractor_cases_reach_their_limit(oracle, case):
    """The strips have level-0 keypoints in the last cell column / row; the quota case returns more than 32 768 keypoints on its
    one level (bit 15 of K3's arrival index) and fills the quota."""
    kps, desc = extractor_want(case, oracle)
    h, w = case["img"].shape
    if case["axis"]:
        side = w if case["axis"] == "x" else h
        assert side == CC.LEVEL_PX
        l0 = kps[kps["octave"] == 0]
        assert l0[case["axis"]].max() >= CC.last_cell_start(side)
        assert len(set(kps["octave"].tolist())) == case["nlevels"]
    else:
        assert len(kps) == CC.LEVEL_KP > 32768


def test_tall_strip_has_no_quadtree_root(oracle):
    """Why the height limit does not run on a 200 x 4095 frame: nIni = round(168 / 4063) = 0, which the oracle reports (-2)."""
    assert CC.tallest_width() == 2064
    with pytest.raises(Exception):
        oracle.OrbOracle(2000, 1.2, 1, 20, 7).extract(CC.banded_frame(3, CC.LEVEL_PX, 200))


def test_bow_vectors_case_depends_on_feature_order():
    c = CC.bow_vectors_capacity_case()
    ids, vals = CC.bow_vectors_reference(c["word"], c["weight"])
    swapped = c["weight"].copy()
    swapped[[5, CC.PLACE_FEATURES - 1]] = swapped[[CC.PLACE_FEATURES - 1, 5]]
    assert CC.bow_vectors_reference(c["word"], swapped)[1].tobytes() != vals.tobytes()
    assert len(c["word"]) == CC.PLACE_FEATURES and ids[0] == 3


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, MC.SCALE, MC.NLEVELS, 20, 7, max_width=MC.W, max_height=MC.H, max_batch=4)
    assert np.array_equal(e.GetScaleFactors(), MC.SF)
    yield e
    e.close()


def refused(call):
    """The call raises PgorbError with PGORB_E_LIMIT."""
    from pilotguru_amd import _lib
    with pytest.raises(_lib.PgorbError) as e:
        call()
    assert e.value.code == _lib.PGORB_E_LIMIT, e.value
    return True


def both_forms_equal_the_reference(cc, ext):
    """The single call and the batched device form (caps exactly at the case's sizes) against the sequential reference."""
    case, want = cc["case"], wanted(cc)
    got = MC.run_gpu(case, ext)
    assert MC.same(want, got), "%s: single call differs from the reference" % cc["name"]
    grids, res = MC.run_gpu_batched([case], ext, "nan", extra=0, qextra=0)
    for (k, b), g in zip(MC._case_frames(case), grids):
        assert MC.same(R.Grid(k, b).csr(), g), "%s: batched grid" % cc["name"]
    assert MC.same(want, res[0]), "%s: batched form differs from the reference" % cc["name"]


def _inert_frame(n, octave=7):
    k = CC._filler_keys(n, np.random.RandomState(n), octave)
    return k, np.zeros((n, 32), np.uint8)


@pytest.mark.gpu
def test_gpu_frame_grid_and_search_for_initialization_at_capacity(ext):
    """cap 16 000, both frames full: k_search_for_initialization's five 16-bit arrays take 160 192 B of the 163 840 B of LDS.
    The grid has no limit of its own (32-bit indices): it takes 16 001 keypoints; the matcher refuses them in both forms."""
    g = CC.grid_capacity_case()
    assert MC.same(wanted(g), MC.run_gpu(g["case"], ext))
    assert MC.same(wanted(g), MC.run_gpu_grid_batched([g["case"]], ext, "huge")[0])
    both_forms_equal_the_reference(CC.sfi_capacity_case(), ext)
    k, d = _inert_frame(CC.KP_MAX + 1, octave=1)
    over = MC.sfi_case("cap", "sfi_one_past", k, d, k, d, win=20)
    assert MC.same(R.Grid(k, CC.BOUNDS).csr(), MC.run_gpu(MC._case("cap", "grid_one_past", "grid", keys=k, bounds=CC.BOUNDS), ext))
    assert refused(lambda: MC.run_gpu(over, ext))
    assert refused(lambda: MC.run_gpu_batched([over], ext, "nan", extra=0))
    small = MC.sfi_case("cap", "sfi_long_f2", k[:3], d[:3], k, d, win=20)         # F2 alone past the limit
    assert refused(lambda: MC.run_gpu(small, ext))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["points", "frame", "keyframe"])
def test_gpu_search_by_projection_on_the_lds_line(ext, kind):
    """The three points of keypoints * 13 + queries * 10 + 256 = 163 840, and one more query on each; 16 001 keypoints."""
    for cap, qcap in CC.SBP_POINTS:
        both_forms_equal_the_reference(CC.sbp_capacity_case(kind, cap, qcap), ext)
        over = CC.sbp_one_past(kind, cap, qcap)
        assert refused(lambda: MC.run_gpu(over, ext))
        assert refused(lambda: MC.run_gpu_batched([over], ext, "nan", extra=0, qextra=0))
    k, d = _inert_frame(CC.KP_MAX + 1)
    c = CC.sbp_capacity_case(kind, 1000, 1)["case"]
    over = dict(c, a=dict(c["a"], keys=k, desc=d, has=np.zeros(len(k), np.uint8)))
    assert refused(lambda: MC.run_gpu(over, ext))
    assert refused(lambda: MC.run_gpu_batched([over], ext, "nan", extra=0, qextra=0))


@pytest.mark.gpu
def test_gpu_search_by_bow_at_capacity(ext):
    """Two frames of 16 000 features; a shared node beyond the 256 features held in registers with members >= 15 990, and one
    whose list positions pass 8 192."""
    cc = CC.bow_capacity_case()
    both_forms_equal_the_reference(cc, ext)
    a = cc["case"]["a"]
    n = CC.KP_MAX + 1
    node = np.concatenate([a["knode"], [3]])
    grow = lambda x: np.concatenate([x, x[-1:]])
    over = dict(cc["case"], a=dict(a, kk=grow(a["kk"]), kd=grow(a["kd"]), kv=grow(a["kv"]), kfv=CC.fv_of(node)))
    assert len(over["a"]["kd"]) == n
    assert refused(lambda: MC.run_gpu(over, ext))
    assert refused(lambda: MC.run_gpu_batched([over], ext, "nan", extra=0))
    over = dict(cc["case"], a=dict(a, fk=grow(a["fk"]), fd=grow(a["fd"]), ffv=CC.fv_of(np.concatenate([a["fnode"], [3]]))))
    assert refused(lambda: MC.run_gpu(over, ext))


@pytest.mark.gpu
def test_gpu_popcount_matcher_at_the_index_field(oracle, ext):
    """nb = 2^20 - 1 train descriptors through pgorb_hamming_best2 and, as a frame of cap 2^20 - 1, through
    pgorb_match_batch_device; 2^20 is refused by both."""
    import torch
    cc = CC.k7_capacity_case()
    a, b = cc["a"], cc["b"]
    want = wanted(dict(cc, case=cc), lambda c: oracle.hamming_best2(c["a"], c["b"]))
    assert ext.matcher_name(len(b)) == "popcount"
    got = ext.hamming_best2(a, b)
    assert all(np.array_equal(w, g) for w, g in zip(want, got))
    cap = len(b)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8)
    desc[0, :len(a)] = torch.from_numpy(a); desc[1] = torch.from_numpy(b)
    desc = desc.cuda()
    n = torch.tensor([len(a), cap], dtype=torch.int32, device="cuda")
    pq, pt = torch.tensor([0], dtype=torch.int32, device="cuda"), torch.tensor([1], dtype=torch.int32, device="cuda")
    bi, b1, b2 = ext.match_batch_device(desc, n, pq, pt)
    torch.cuda.synchronize()
    na = len(a)
    assert np.array_equal(bi[0, :na].cpu().numpy(), want[0])
    assert np.array_equal(b1[0, :na].cpu().numpy().view(np.uint16), want[1]) and np.array_equal(b2[0, :na].cpu().numpy().view(np.uint16), want[2])
    del desc, bi, b1, b2
    assert refused(lambda: ext.hamming_best2(a, np.zeros((cap + 1, 32), np.uint8)))
    assert refused(lambda: ext.match_batch_device(torch.empty((1, cap + 1, 32), dtype=torch.uint8, device="cuda"), n, pq, pq))


@pytest.mark.gpu
def test_gpu_bow_node_matchers_between_key_frames_at_capacity(ext):
    """SearchByBoW(KF, KF) and SearchForTriangulation on two key frames of 16 000 features with the node layout of the frame form."""
    import loop_cases as LC
    import triangulation_cases as TC
    cc = CC.kfbow_capacity_case()
    want = wanted(cc, LC.run_ref1)
    assert LC.same(want, LC.run_gpu1(cc["case"], ext))
    assert LC.same(want, LC.run_gpu1_batched([cc["case"]], ext, extra=0)[0])
    over = CC.kfbow_capacity_case(cap=CC.KP_MAX + 1)["case"]
    assert refused(lambda: LC.run_gpu1(over, ext)) and refused(lambda: LC.run_gpu1_batched([over], ext, extra=0))
    cc = CC.tri_capacity_case()
    want = wanted(cc, TC.run_reference)
    assert TC.same(want, TC.run_gpu(cc["case"], ext))
    res, mh, n1 = TC.run_gpu_batched([cc["case"]], ext, extra=0)
    assert TC.same(want, res[0])
    over = CC.tri_capacity_case(cap=CC.KP_MAX + 1)["case"]
    assert refused(lambda: TC.run_gpu(over, ext)) and refused(lambda: TC.run_gpu_batched([over], ext, extra=0))


@pytest.mark.gpu
def test_gpu_fuse_and_loop_projection_matchers_in_a_key_frame_of_16000(ext):
    """Fuse, Fuse(Scw), SearchByProjection(Scw) and SearchBySim3 with the winners in slots >= 15 990; 16 001 keypoints refused."""
    import fuse_cases as FC
    import loop_cases as LC
    cc = CC.fuse_capacity_case()
    want = wanted(cc, FC.run_reference)
    assert FC.same(want, FC.run_gpu(cc["case"], ext))
    got = FC.run_gpu_batched([cc["case"]], ext, extra=0)[0]
    assert FC.same(want, got[:5]) and np.all(got[5] == -9)
    over = CC.fuse_capacity_case(total=CC.KP_MAX + 1)["case"]
    assert refused(lambda: FC.run_gpu(over, ext)) and refused(lambda: FC.run_gpu_batched([over], ext, extra=0))
    for which, cases, ref, run in ((3, CC.ps3_capacity_cases(), LC.run_ref3, LC.run_gpu3), (4, [CC.fs3_capacity_case()], LC.run_ref4, LC.run_gpu4)):
        for cc in cases:
            want = wanted(cc, ref)
            assert LC.same(want, run(cc["case"], ext)), cc["name"]
            got = LC.run_gpu_batched([cc["case"]], ext, which, extra=0)[0]
            assert LC.same(want, got[:-1]) and np.all(got[-1] == LC.SENTINEL), cc["name"]
    over = CC.ps3_capacity_cases(total=CC.KP_MAX + 1)[0]["case"]
    for which, run in ((3, LC.run_gpu3), (4, LC.run_gpu4)):
        assert refused(lambda: run(over, ext)) and refused(lambda: LC.run_gpu_batched([over], ext, which, extra=0))
    cc = CC.sim3_capacity_case()
    want = wanted(cc, LC.run_ref2)
    assert LC.same(want, LC.run_gpu2(cc["case"], ext))
    got = LC.run_gpu2_batched([cc["case"]], ext, extra=0)[0]
    assert LC.same(want, got[:2])
    over = CC.sim3_capacity_case(total=CC.KP_MAX + 1)["case"]
    assert refused(lambda: LC.run_gpu2(over, ext)) and refused(lambda: LC.run_gpu2_batched([over], ext, extra=0))


def _cnm_same(want, got):
    import mapping_cases as MP
    pts, cnt, F, ep, h = want
    gp, gc, gF, gep, gh = got[:5]
    return (MP.same_point_lists(pts, gp) and [int(x) for x in cnt] == [int(x) for x in gc] and
            np.asarray(F, np.float32).tobytes() == np.asarray(gF, np.float32).tobytes() and
            np.asarray(ep, np.float32).tobytes() == np.asarray(gep, np.float32).tobytes() and np.array_equal(np.asarray(h), np.asarray(gh)))


@pytest.mark.gpu
def test_gpu_create_new_map_points_with_64_neighbours_and_16000_keypoints(ext):
    """KF1 of 16 000 keypoints and all 64 neighbour slots, the last of which is the first to triangulate some keypoints;
    65 neighbours and 16 001 keypoints (in KF1, in a neighbour) are refused."""
    import mapping_cases as MP
    cc = CC.cnm_capacity_case()
    KF1, neigh = cc["case"]
    want = wanted(cc, lambda c: MP.run_reference(*c))
    assert _cnm_same(want, MP.run_gpu(KF1, neigh, ext))
    assert _cnm_same(want, MP.run_gpu_batched([(KF1, neigh)], ext, extra=0)[0])
    small = neigh[CC.CNM_NEIGH - 1]
    with pytest.raises(ValueError):                                            # the Python mirror counts the neighbours itself ...
        MP.run_gpu(small, neigh + [small], ext)
    from pilotguru_amd import _lib
    z = np.zeros(4096, np.uint8)
    p = C.c_void_p(z.ctypes.data)                                              # ... and so does the library, before it reads anything
    assert ext._L.pgorb_create_new_map_points(ext._h, p, p, p, 0, p, p, p, 0, p, CC.CNM_NEIGH + 1, *([p] * 15)) == _lib.PGORB_E_LIMIT
    assert refused(lambda: MP.run_gpu_batched([(small, neigh[:3])], ext, M=CC.CNM_NEIGH + 1))
    big, slots = CC.cnm_capacity_case(total=CC.KP_MAX + 1)["case"]
    assert refused(lambda: MP.run_gpu(big, slots[:2], ext))
    assert refused(lambda: MP.run_gpu(small, [dict(big, median=np.float32(4.0))], ext))
    assert refused(lambda: MP.run_gpu_batched([(big, slots[:2])], ext, extra=0))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["reloc", "loop"])
def test_gpu_place_recognition_at_65536_frames_and_65535_queries(ext, form):
    """A table of 65 536 frames with the candidates in rows 65 535 and 32 768 (single call, and both query rows in one batch);
    65 535 queries over a small table in one batch; 65 537 frames and 65 536 queries are refused."""
    import torch
    from pilotguru_amd import _lib
    from test_place_recognition import _stream, _tp, differs, gpu_batch, gpu_single
    cc = CC.place_capacity_case(form)
    t = cc["case"]
    wants = {r: wanted(dict(cc, name="%s/q%d" % (cc["name"], r)), lambda tt, r=r: tt.reference(r)) for r in (0, 1)}
    assert wants[0]["cand"] == [CC.half(CC.PLACE_FRAMES), CC.PLACE_FRAMES - 1]
    got = gpu_single(ext, t.csr(0), form)
    assert not differs(got, wants[0]) and got["ncand"] == 2, (got["cand"], got["stats"])
    for r, got in zip((0, 1, 0), gpu_batch(ext, t.padded([0, 1, 0]), form, 64)):
        assert not differs(got, wants[r]) and got["ncand"] == len(wants[r]["cand"]), (r, got["cand"], got["stats"])
    many = CC.place_many_queries_case(form)
    mt, rows = many["case"], many["query_rows"]
    per = {r: mt.reference(r) for r in (0, 1)}
    assert len(rows) == CC.PLACE_QUERIES and all(len(per[r]["cand"]) > 0 for r in per)
    out = gpu_batch(ext, mt.padded(rows), form, 8)
    bad = [q for q, (r, got) in enumerate(zip(rows, out)) if differs(got, per[r]) or got["ncand"] != len(per[r]["cand"])]
    assert not bad, (len(bad), bad[:5], bad[-5:])
    # one past: the gates answer before any pointer is read
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    L, h, E = ext._L, ext._h, _lib.PGORB_E_LIMIT
    for nframes, nq in ((CC.PLACE_FRAMES + 1, 1), (8, CC.PLACE_QUERIES + 1)):
        if form == "reloc":
            rc = L.pgorb_detect_relocalization_candidates_batch_device(h, _tp(z), _tp(z), _tp(z), nframes, 4, _tp(z), _tp(z), _tp(z), nq, None,
                                                                       _tp(z), 8, _tp(z), None, None, None, _stream())
        else:
            rc = L.pgorb_detect_loop_candidates_batch_device(h, _tp(z), _tp(z), _tp(z), nframes, 4, _tp(z), _tp(z), _tp(z), nq, _tp(z), _tp(z),
                                                             _tp(z), 0, _tp(z), 8, _tp(z), None, None, None, _stream())
        assert rc == E, (nframes, nq, rc)
    small = mt.csr(0)
    a = lambda k: C.c_void_p(small[k].ctypes.data)
    cand = np.zeros(8, np.int32)
    if form == "reloc":
        rc = L.pgorb_detect_relocalization_candidates(h, CC.PLACE_FRAMES + 1, a("bow_start"), a("bow_id"), a("bow_val"), a("in_db"), a("neigh_start"),
                                                      a("neigh"), 0, None, C.c_void_p(cand.ctypes.data), 8, None, None)
    else:
        rc = L.pgorb_detect_loop_candidates(h, CC.PLACE_FRAMES + 1, a("bow_start"), a("bow_id"), a("bow_val"), a("in_db"), a("neigh_start"),
                                            a("neigh"), 0, 0.0, None, 0, C.c_void_p(cand.ctypes.data), 8, None, None, None)
    assert rc == E, rc


@pytest.mark.gpu
def test_gpu_bow_vectors_at_8192_features(ext, tmp_path):
    """k_bow_vectors with every one of its 8 192 slots in use (8 ranks per thread), against the sums written out by hand."""
    import torch
    import vocab_cases as VC
    from pilotguru_amd import vocab as V
    from test_place_recognition import _gpu_bow_vectors
    tree = VC.random_tree(4, 20, 3)._replace(weighting=1)                       # L1_NORM with TF: the kernel's contract
    V.ORBVocabulary(text_file=VC.write_text(tree, os.path.join(str(tmp_path), "tf.txt"))).upload(ext)
    c = CC.bow_vectors_capacity_case()
    cap = CC.PLACE_FEATURES
    word = torch.from_numpy(np.stack([c["word"], c["word"][::-1].copy()]).view(np.int32)).cuda()
    weight = torch.from_numpy(np.stack([c["weight"], c["weight"][::-1].copy()])).cuda()
    n = torch.tensor([cap, cap], dtype=torch.int32, device="cuda")
    bid, bval, nb = _gpu_bow_vectors(ext, word, weight, n, cap)
    for f, (w, x) in enumerate(((c["word"], c["weight"]), (c["word"][::-1], c["weight"][::-1]))):
        ids, vals = CC.bow_vectors_reference(w, x)
        assert nb[f] == len(ids) and np.array_equal(bid[f, :nb[f]], ids) and bval[f, :nb[f]].tobytes() == vals.tobytes(), f


@pytest.mark.gpu
@pytest.mark.parametrize("case", CC.extractor_capacity_cases(), ids=lambda c: c["name"])
def test_gpu_extractor_at_the_level_limits(oracle, case):
    """Level sides of 4 095 px and a level quota of 65 533, host frame and resident batch, byte for byte against the oracle."""
    import pilotguru_amd as pg
    import torch
    from pilotguru_amd.orb import KEYPOINT_DTYPE
    okp, odesc = extractor_want(case, oracle)
    h, w = case["img"].shape
    e = pg.ORBextractor(case["nfeatures"], 1.2, case["nlevels"], 20, 7, max_width=w, max_height=h)
    try:
        kp, desc = e(case["img"])
        assert len(kp) == len(okp) and kp.tobytes() == okp.tobytes() and np.array_equal(desc, odesc)
        dk, dd, dn = e.extract_batch_device(torch.from_numpy(case["img"][None]).cuda())
        e.check_async()
        torch.cuda.synchronize()
        m = int(dn[0])
        assert m == len(okp) and dk[0, :m].cpu().numpy().view(KEYPOINT_DTYPE).reshape(-1).tobytes() == okp.tobytes()
        assert np.array_equal(dd[0, :m].cpu().numpy(), odesc)
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_extractor_refuses_one_past_its_limits():
    """max_width / max_height 4 096 are refused when the context is made, a level quota of 65 534 when the frame is planned."""
    import pilotguru_amd as pg
    assert refused(lambda: pg.ORBextractor(1000, 1.2, 1, 20, 7, max_width=CC.LEVEL_PX + 1, max_height=200))
    assert refused(lambda: pg.ORBextractor(1000, 1.2, 1, 20, 7, max_width=200, max_height=CC.LEVEL_PX + 1))
    e = pg.ORBextractor(CC.LEVEL_KP + 1, 1.2, 1, 20, 7, max_width=320, max_height=240)
    try:
        assert refused(lambda: e(CC.noise_frame(4, 240, 320)))
    finally:
        e.close()


if __name__ == "__main__":                      # the table of profiles/capacity_tests.txt: every case, what it fills, its reference's seconds
    from oracle import orb_oracle
    orb_oracle.build()
    rows = []
    for fam, cases, ref in families():
        for cc in cases:
            want_of(cc, ref)
            rows.append((cc["name"], cc["size"], cc["fills"]))
    k7 = CC.k7_capacity_case()
    wanted(dict(k7, case=k7), lambda c: orb_oracle.hamming_best2(c["a"], c["b"]))
    rows.append((k7["name"], k7["size"], k7["fills"]))
    for case in CC.extractor_capacity_cases():
        extractor_want(case, orb_oracle)
        rows.append((case["name"], case["size"], case["fills"]))
    for name, size, fills in rows:
        print("%-34s %7.3f s  %s | %s" % (name, REFERENCE_SECONDS[name], size, fills))
    print("total %.3f s" % sum(REFERENCE_SECONDS.values()))
