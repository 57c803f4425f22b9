"""pgorb_optimize_essential_graph (pilotguru_amd/csrc/essential_graph.hip): Optimizer::OptimizeEssentialGraph on the GPU against the
dense reference of tests/eg_reference.py on the constructed graphs of tests/eg_cases.py.

The CPU tests anchor the reference's reading of g2o (log against exp, the numeric Jacobian against an independent difference, one
damped solve against numpy.linalg.solve, the block skyline against the dense factorisation bit for bit, the edge derivation against
a literal transcription with std::map / std::set semantics, a consistent graph, a drifted loop of known drift), show what each rule
mutant changes, and keep tests/golden/eg_spread.json up to date.  The GPU tests compare the single call and the device form with
the reference (integers exactly, floats and doubles by eg_cases.bounds: the larger of 2 ulps and 16 x the recorded spread of the
case), the two forms with each other byte for byte, a repeat, a second stream and a context that ran LBA in between, the chain
into pgorb_refresh_map_points_batch_device, NOTHING and NONFINITE, the refusals and the capacities.

WHAT GUARDS WHAT.  Seven CPU tests exercise tests/eg_reference.py alone -- log and exp, the numeric Jacobian, the solve and the
skyline, the edge derivation, the consistent graph, the drifted loop, the equivalent mutant -- together with the spread file and the
mutants: they anchor the reference and pass without the library.  The library is guarded by the presence test, the C++ mirror's
compilation and the mirror's refusals (CPU; they fail without the new symbols and mirrors) and by every test marked gpu.

On the MI355X every integer of every case equalled the reference's; Tcw, Ow and pos equalled it bit for bit in every case but
"filters" (one float ulp in Tcw against a bound of 4.4e3); the largest differences in double were 1.9e7 ulps in sim3 (bound 5.5e10),
1.4e7 in an edge's relative Sim3 (bound 9.9e10) and 1.5e8 in an edge's chi2 (bound 4.1e11), all on that case: the device's libm is not glibc's and the 1e-9 quotient amplifies it."""
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
import eg_cases as EC  # noqa: E402
import eg_reference as ER  # noqa: E402
import map_point_reference as MR  # noqa: E402
from optsim3_reference import Sim3, sim3_exp, sim3_mul  # noqa: E402

f32, f64 = np.float32, np.float64
NAMES = ("pgorb_optimize_essential_graph", "pgorb_optimize_essential_graph_device")
LM = ER.LibM2(False)


# ---------------------------------------------------------------- presence
def test_symbols_and_mirrors_are_present():
    """The two entry points are exported and refuse a NULL context; the mirrors and the constants exist and agree with the header."""
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    z = np.zeros(64, f64)
    p = C.c_void_p(z.ctypes.data)
    assert L.pgorb_optimize_essential_graph(None, 0, p, p, None, 0, 0, 0, None, None, None, None, 0, p, p, p, p, p, p, p, 100, 20, 0, p, None, p, p, p,
                                            None, None) == _lib.PGORB_E_ARG
    assert L.pgorb_optimize_essential_graph_device(None, 0, p, p, None, 0, 0, 0, None, None, None, None, 0, p, p, p, p, 0, p, p, p, 0, 100, 20, 0, p,
                                                   None, p, p, p, None, p, None) == _lib.PGORB_E_ARG
    assert (pg.EG_NOTHING, pg.EG_NONFINITE, pg.EG_LIMIT, pg.EG_INFO) == (ER.EG_NOTHING, ER.EG_NONFINITE, ER.EG_LIMIT, 10)
    assert pg.EG_MAX_KF >= 2048 and pg.EG_MAX_EDGES >= 32768
    assert pg.SIM3D_DTYPE == EC.SIM3D_DTYPE and pg.SIM3D_DTYPE.itemsize == 64 and pg.EG_EDGE_DTYPE.itemsize == 24
    assert pg.KF_POSE_DTYPE == EC.KF_POSE_DTYPE and pg.MAP_POINT_DTYPE == EC.MAP_POINT_DTYPE
    assert callable(pg.Optimizer.OptimizeEssentialGraph) and callable(pg.Optimizer.OptimizeEssentialGraph_device)
    hpp = open(os.path.join(ROOT, "pilotguru_amd", "host", "orb_extractor.hpp")).read()
    assert "EssentialGraphResult OptimizeEssentialGraph(" in hpp and "pgorb_optimize_essential_graph(ctx_" in hpp
    hdr = open(os.path.join(ROOT, "include", "pgorb.h")).read()
    assert all(("int  %s(" % n) in hdr for n in NAMES)
    for text in ("#define PGORB_EG_INFO           10", "#define PGORB_EG_MAX_KF         %d" % pg.EG_MAX_KF, "#define PGORB_EG_MAX_EDGES      %d" % pg.EG_MAX_EDGES,
                 "#define PGORB_EG_MAX_ENVELOPE_BLOCKS %d" % pg.EG_MAX_ENVELOPE_BLOCKS, "#define PGORB_EG_LIMIT          4"):
        assert text in hdr, text
    src = open(os.path.join(ROOT, "pilotguru_amd", "csrc", "optimize_sim3.hip")).read()
    assert '#include "g2o_sim3.h"' in src and "os_exp(const double" not in src, "the Sim3 helpers live in g2o_sim3.h"


def test_cpp_mirror_compiles():
    """host/orb_extractor.hpp with the new mirror is valid C++17 (syntax only: no device is needed)."""
    src = ("#include \"orb_extractor.hpp\"\nint main() { pgorb::Optimizer o(nullptr); pgorb::EssentialGraph g; std::vector<pgorb_map_point> p;\n"
           "  if (g.kfId.size() == 1) o.OptimizeEssentialGraph(g, p, {}); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "pilotguru_amd", "host"), "-x", "c++", "-"], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


# ---------------------------------------------------------------- anchors of the reading
def test_log_inverts_exp_and_exp_of_log_maps_points_alike():
    """log(exp(u)) == u and exp(log(S)) maps points as S does, in every branch pair the two functions share.  Sim3(Vector7d) takes
    its small-angle branch below theta = 1e-5, Sim3::log below 1 - cos(theta) = 1e-5 (theta = 4.5e-3): between the two, with
    |sigma| >= 1e-5, log uses sim3.h:199's B = (sigma^2/2 - sigma + 1) s / sigma^3 (of the order of 1 / sigma^3, not 1/6) against
    exp's general B, and is no inverse.  The reference restates that as the source has it; the test stays outside that window and
    shows it once."""
    rng = np.random.RandomState(3)
    for theta, sigma in ((0.7, 0.3), (0.02, 0.3), (0.7, 1e-7), (0.02, 0.0), (1e-7, 0.3), (1e-7, 1e-7), (0.0, 0.0), (2e-3, 1e-7), (2.5, -0.4)):
        for _ in range(4):
            ax = rng.randn(3)
            u = np.concatenate([ax / np.linalg.norm(ax) * theta, rng.uniform(-3, 3, 3), [sigma]])
            S = sim3_exp(u, LM)
            v = ER.sim3_log(S, LM)
            # log's first-order branch (theta < 4.5e-3) takes omega = sin(theta) * axis and A = 1/2, B = 1/6: relative theta^2 / 6 and
            # theta^2 / 24, so theta^3 / 6 * |P| + theta^3 / 24 * |upsilon| with |P| <= 8.7, |upsilon| <= 5.2: below 2 theta^3
            tol = 1e-12 + (10 * theta ** 3 if theta < 5e-3 else 0.0)
            assert np.abs(v - u).max() <= tol, (theta, sigma, np.abs(v - u).max())
            S2 = sim3_exp(v, LM)
            P = rng.uniform(-5, 5, 3)
            assert np.abs(ER.sim3_map(S, P) - ER.sim3_map(S2, P)).max() <= tol, (theta, sigma)
    u = np.array([1e-3, 2e-3, -1e-3, 3e-3, 1e-3, 2e-3, 1.5e-3])         # inside the window: g2o's own log departs from its exp
    assert np.abs(ER.sim3_log(sim3_exp(u, LM), LM) - u).max() > 1e-3
    many = ER.stack([sim3_exp(rng.randn(7) * 0.3, LM) for _ in range(9)])
    one = np.stack([ER.sim3_log(Sim3(many.q[:, k], many.t[:, k], many.s[k]), LM) for k in range(9)], 1)
    assert np.array_equal(ER.sim3_log(many, LM), one), "one transform per edge equals one at a time, bit for bit"


def test_numeric_jacobian_equals_an_independent_difference_at_a_larger_step():
    """BaseBinaryEdge::linearizeOplus (delta = 1e-9) against central differences of the reference's own computeError at h = 1e-5.
    The errors are logs of magnitude M <= 1 built from translations of magnitude T <= 8, so one error carries a rounding of about
    eps * T: the 1e-9 quotient carries eps * T / 1e-9 = 1.8e-6, the h quotient eps * T / h = 1.8e-10 plus h^2 times a third
    derivative (of the order of T).  The bound is ten times their sum.  The vertices are moved away from the measurements first:
    an error whose rotation is below 4.5e-3 rad and whose |log scale| reaches 1e-5 falls into the window where Sim3::log is no
    inverse of Sim3(Vector7d) (the test above), and there a step of 1e-5 and a step of 1e-9 in the scale see different functions."""
    c = EC.case("ring12")
    vscw, edges, meas = ER.derive(c)
    rng = np.random.RandomState(8)
    vscw = [sim3_mul(sim3_exp(rng.uniform(-0.2, 0.2, 7), LM), S) for S in vscw]      # every error far from the identity: see below
    Cm = ER.stack(meas)
    Si, Sj = ER.stack([vscw[e[0]] for e in edges]), ER.stack([vscw[e[1]] for e in edges])
    assert np.abs(ER.edge_errors(Cm, Si, Sj, LM)[:3]).max(0).min() > 1e-2, "no error rotation inside Sim3::log's first-order window"
    Ji, Jj = ER.jacobians(Cm, Si, Sj, False, LM, ER.REFERENCE)
    h, T, eps = 1e-5, 8.0, np.finfo(f64).eps
    bound = 10.0 * (eps * T / 1e-9 + eps * T / h + h * h * T)
    worst = 0.0
    for side, J in ((0, Ji), (1, Jj)):
        for d in range(7):
            err = []
            for s in (+h, -h):
                u = np.zeros(7)
                u[d] = s
                E = sim3_exp(u, LM)
                err.append(ER.edge_errors(Cm, sim3_mul(E, Si), Sj, LM) if side == 0 else ER.edge_errors(Cm, Si, sim3_mul(E, Sj), LM))
            diff = np.abs((err[0] - err[1]) / (2 * h) - J[:, d]).max()
            worst = max(worst, diff)
            assert diff <= bound, (side, d, diff, bound)
    assert 0.0 < worst
    Jf, _ = ER.jacobians(Cm, Si, Sj, True, LM, ER.REFERENCE)
    assert not Jf[:, 6].any() and np.array_equal(Jf[:, :6], Ji[:, :6]), "under _fix_scale oplusImpl zeroes update[6]: the column is 0"


def test_one_damped_solve_equals_numpy_and_the_skyline_equals_the_dense_factorisation_bit_for_bit():
    """The first system of every case, damped: the index-order Cholesky (both forms) against numpy.linalg.solve, and the block
    skyline (only blocks inside the envelope are touched) against the dense LLT bit for bit, with the envelope the device reports."""
    for name in EC.NAMES:
        r = EC.reference(name)
        if r["H0"] is None:
            continue
        H, b = r["H0"], r["b0"]
        assert np.array_equal(H, H.T)
        for lam in (1e-16, 3.7):
            Hl = H + lam * np.eye(len(b))
            x, ok = ER.chol_solve(Hl, b, ER.DEVICE_FORM)
            x2, ok2 = ER.chol_solve(Hl, b, ER.Form(chol="ldlt"))
            xs, oks, env = ER.skyline_solve(Hl, b, len(b) // 7)
            assert oks == ok and np.array_equal(xs, x), (name, lam)
            if lam > 1 and ok and ok2:
                want = np.linalg.solve(Hl, b)
                scale = np.abs(want).max()
                assert np.abs(x - want).max() <= 1e-9 * scale and np.abs(x2 - want).max() <= 1e-9 * scale, (name, lam)
        n = len(b) // 7
        assert n <= env <= n * (n + 1) // 2
        if name == "ring12":
            assert env == 1 + 2 + 3 * 8 + 3 == 30           # rows of one, two and three blocks, and cur's row: parent, covisible, diagonal
        if name == "hub80":
            assert env > 70 * 8, "seventy long rows over the same columns"
        if name == "two_loops":
            assert env > 3 * n, "the previous loop edge and the new connection make two long rows"


def _pose_close(r, c, depth=0):
    """pose_out == pose within 4 (1 + depth) float ulps at the scale of the record's largest entry.  A float rotation is orthonormal
    to an ulp at 1 an entry; R -> quaternion -> R in double returns its orthonormal part and the result is rounded to float once
    more: 4 ulps.  Sim3::inverse conjugates the quaternion, which inverts a unit quaternion only: the quaternion of a float rotation
    has norm 1 +- 2 float ulps, so every measurement S_j * S_i^-1 starts with an error of that order although it was made from the
    vertices, and the optimum (zero error along a spanning tree) moves a vertex by at most the sum of those errors over its `depth`
    edges to the fixed vertex."""
    tol = 4 * np.finfo(f32).eps * (1 + np.asarray(depth, f64)) * np.maximum(np.abs(c["pose"]["Tcw"]).max(1), 1.0)
    worst = np.abs(r["Tcw"].astype(f64) - c["pose"]["Tcw"]).max(1) / tol
    print("pose_out against pose: %.3g of the bound at key frame %d" % (worst.max(), int(worst.argmax())))
    return bool((worst <= 1.0).all())


class _KF:
    def __init__(self, i, mnid, bad):
        self.i, self.mnId, self.bad, self.parent, self.children, self.loop_edges, self.covis = i, int(mnid), bool(bad), None, set(), set(), []

    def __lt__(self, o):                                      # std::set<KeyFrame*> / std::map<KeyFrame*, ...> order: by address
        return self.i < o.i


def _literal_edges(c):
    """Optimizer.cc:847-983 line by line over KeyFrame objects, std::map / std::set as sorted containers, sInsertedEdges as a set of
    id pairs; a bad key frame has no vertex (optimizer.vertex() == NULL: no edge)."""
    kfs = [_KF(i, c["kf_id"][i], c["kf_bad"][i]) for i in range(c["nkf"])]
    for i, k in enumerate(kfs):
        p = int(c["parent"][i])
        if p >= 0:
            k.parent = kfs[p]
            kfs[p].children.add(k)
        k.loop_edges = {kfs[j] for j in c["loop_edge"][c["loop_edge_start"][i]:c["loop_edge_start"][i + 1]]}
        k.covis = [(kfs[c["covis"][q]], int(c["covis_weight"][q])) for q in range(c["covis_start"][i], c["covis_start"][i + 1])]
    loop_connections, weight = {}, {}
    for i, j, w in c["loop_conn"]:                            # the caller's map-then-set iteration order is the list order
        loop_connections.setdefault(kfs[i], []).append(kfs[j])
        weight[(i, j)] = int(w)
    cur, loop, min_feat = kfs[c["cur_kf"]], kfs[c["loop_kf"]], c["min_feat"]
    vertex = lambda k: None if k.bad else k
    inserted, edges = set(), []
    for pKF, conns in loop_connections.items():
        for pKFj in conns:
            if (pKF.mnId != cur.mnId or pKFj.mnId != loop.mnId) and weight[(pKF.i, pKFj.i)] < min_feat:
                continue
            if vertex(pKF) is None or vertex(pKFj) is None:
                continue
            edges.append((pKF.i, pKFj.i, 0))
            inserted.add((min(pKF.mnId, pKFj.mnId), max(pKF.mnId, pKFj.mnId)))
    for pKF in kfs:
        if pKF.bad:
            continue
        if pKF.parent is not None and vertex(pKF.parent) is not None:
            edges.append((pKF.i, pKF.parent.i, 1))
        for pLKF in sorted(pKF.loop_edges, key=lambda k: [int(x) for x in c["loop_edge"][c["loop_edge_start"][pKF.i]:c["loop_edge_start"][pKF.i + 1]]].index(k.i)):
            if pLKF.mnId < pKF.mnId and vertex(pLKF) is not None:
                edges.append((pKF.i, pLKF.i, 2))
        for pKFn, w in pKF.covis:
            if w < min_feat:                                  # GetCovisiblesByWeight(minFeat)
                continue
            if pKFn is not pKF.parent and pKFn not in pKF.children and pKFn not in pKF.loop_edges:
                if not pKFn.bad and pKFn.mnId < pKF.mnId:
                    if (min(pKF.mnId, pKFn.mnId), max(pKF.mnId, pKFn.mnId)) in inserted:
                        continue
                    edges.append((pKF.i, pKFn.i, 3))
    return edges


def test_edge_derivation_equals_a_literal_transcription():
    seen = set()
    for name in EC.NAMES:
        c = EC.case(name)
        _, edges, _ = ER.derive(c)
        assert edges == _literal_edges(c), name
        seen |= {e[2] for e in edges}
    assert seen == {0, 1, 2, 3}
    r = EC.reference("filters")
    e = set(r["edges"])
    assert (11, 0, 0) in e and (11, 1, 0) in e and (1, 10, 0) in e and not any(x in e for x in ((11, 2, 0), (10, 0, 0), (0, 11, 0)))
    assert (9, 2, 2) in e and (9, 10, 2) not in e and (2, 9, 2) not in e and (10, 9, 2) in e
    assert (9, 6, 3) in e and (4, 1, 3) in e
    assert not any(x in e for x in ((9, 5, 3), (9, 2, 3), (9, 8, 3), (9, 10, 3), (9, 11, 3), (11, 0, 3), (11, 1, 3), (11, 3, 3), (10, 1, 3), (7, 3, 3)))
    assert (3, 7, 1) in e
    iso = EC.reference("isolated")
    assert not any(5 in x[:2] for x in iso["edges"]) and iso["Tcw"][5].tobytes() == EC.case("isolated")["pose"]["Tcw"][5].tobytes()
    assert iso["sim3"][5].any(), "a key frame without an edge keeps its pose and reports its input estimate"


def test_a_consistent_graph_returns_its_input():
    """Every measurement is generated from the poses the vertices start at: chi2 is rounding, and pose_out is the input through
    R -> quaternion -> R in double, rounded to float."""
    c = EC.case("consistent")
    r = EC.reference("consistent")
    # a float rotation is orthonormal to 6e-8 an entry and Sim3 never renormalises its quaternion: an edge's log error is below 1e-6 a
    # component, its chi2 below 7e-12
    assert r["status"] == 0 and r["ret"] == 11 and r["chi2"].max() < 7e-12
    assert _pose_close(r, c) and np.abs(r["pos"] - c["points"]["pos"]).max() <= 4 * np.finfo(f32).eps * 8


def test_a_drifted_loop_of_known_drift_recovers_the_generating_poses():
    """Vertices start at G_i * D_i (D known, identity at cur and loop); every normal edge measures G_j * G_i^-1 (NonCorrectedSim3 =
    G_i * K) and the loop connection G_loop * G_cur^-1, so the optimum is G exactly and chi2 there is 0.  Gauss-Newton from a drift
    of at most 0.13 rad / 0.13 in log scale converges quadratically; after four iterations the reference is at chi2 < 1e-20, and a
    chi2 of c bounds every entry of every log error by sqrt(c): the bound 1e-8 on the Sim3 entries (translations <= 8) follows."""
    for name, fix in (("drift_known", False), ("drift_known_fix_scale", True)):
        c, r = EC.case(name), EC.reference(name)
        assert r["status"] == 0 and r["iterations"] == 4 and r["trials"] == 4 and r["chi2"].sum() < 1e-20
        start = max(np.abs(np.concatenate([c["D"][i].q, c["D"][i].t, [c["D"][i].s]]) - np.concatenate([c["G"][i].q, c["G"][i].t, [c["G"][i].s]])).max()
                    for i in range(c["nkf"]))
        assert start > 1e-2
        for i in range(c["nkf"]):
            G = c["G"][i]
            assert np.abs(r["sim3"][i] - np.concatenate([G.q, G.t, [G.s]])).max() <= 1e-8, (name, i)
            Tcw, _ = ER.to_pose(G)
            assert np.abs(r["Tcw"][i] - Tcw).max() <= 2 * np.finfo(f32).eps * 8


# ---------------------------------------------------------------- the spread file, the forms and the mutants
def test_spread_file_is_up_to_date_and_integers_agree_under_every_form():
    """tests/golden/eg_spread.json (tests/golden/make_eg_spread.py writes it) holds what the reference shows now, and every form of
    the reference gives every case the same status, return value, iterations, trials and edges."""
    rec = EC.load_spread()
    assert sorted(rec) == sorted(EC.NAMES)
    for n in EC.NAMES:
        now = EC.measure_spread(n)
        assert now["integers_agree"] and rec[n]["integers_agree"], n
        for k in EC.FLOAT_OUTPUTS + EC.DOUBLE_OUTPUTS:
            assert abs(now[k] - rec[n][k]) <= 1e-3 * max(now[k], rec[n][k]) + 1e-300, (n, k, now[k], rec[n][k])


def _as_got(r):
    return {k: r[k] for k in ("status", "ret", "iterations", "trials", "free", "vertices", "kinds", "edges", "Tcw", "Ow", "pos", "sim3", "chi2")}


# where each mutant must show (a compared output outside the bounds of the case), on the CPU
MUTANT_CASES = {
    "no_cur_loop_exception": "ring12", "minfeat_at_equal_skipped": "filters", "inserted_edges_not_deduped": "filters",
    "loop_edges_any_id": "filters", "covisibles_any_id": "filters", "covisible_parent_kept": "filters", "covisible_child_kept": "filters",
    "covisible_loop_edge_kept": "filters", "loop_conn_from_non_corrected": "ring12", "normal_edges_from_vscw": "ring12", "loop_kf_free": "ring12",
    "lambda_from_diagonal": "ring12", "loop_connections_last": "kf40", "t_not_divided_by_s": "ring12",
    "points_from_non_corrected": "ring12",
}


# a mutant that cannot change an output; test_the_equivalent_mutant_changes_nothing_and_why shows why
EQUIVALENT = ("x6_not_zeroed",)


def test_every_mutant_changes_a_compared_output():
    assert sorted(MUTANT_CASES) + sorted(EQUIVALENT) == sorted(ER.MUTANTS)
    for m, name in MUTANT_CASES.items():
        bad, _ = EC.compare(name, _as_got(EC.reference(name, rules=ER.MUTANTS[m])))
        assert bad, "%s changes nothing that is compared on %s" % (m, name)


def test_the_equivalent_mutant_changes_nothing_and_why():
    """Under _fix_scale every perturbed estimate of column 6 is the estimate itself, so the Jacobian's column 6 is exactly 0: row and
    column 6 of every block of H are 0 but for lambda on the diagonal, b's entry is 0, and the solver's x[6] is 0 / lambda = 0
    before oplusImpl writes its own zero there.  computeScale sees the same x either way."""
    for name in ("ring12_fix_scale", "drift_known_fix_scale"):
        r = EC.reference(name)
        assert not r["H0"][6::7].any() and not r["H0"][:, 6::7].any() and not r["b0"][6::7].any()
        m = EC.reference(name, rules=ER.MUTANTS["x6_not_zeroed"])
        assert all(np.array_equal(np.asarray(m[k]), np.asarray(r[k])) for k in ("Tcw", "Ow", "pos", "sim3", "chi2")) and m["trials"] == r["trials"]


# ---------------------------------------------------------------- the mirror's checks, without a device
def _call(ext, c, **kw):
    import pilotguru_amd as pg
    a = dict(kf_id=c["kf_id"], poses=c["pose"], loop_kf=c["loop_kf"], cur_kf=c["cur_kf"], parent=c["parent"], loop_conn=c["loop_conn"],
             loop_edge_start=c["loop_edge_start"], loop_edge=c["loop_edge"], covis_start=c["covis_start"], covis=c["covis"],
             covis_weight=c["covis_weight"], points=c["points"], point_ref_kf=c["point_ref_kf"], kf_bad=c["kf_bad"], point_bad=c["point_bad"],
             has_corrected=c["has_corrected"], corrected=c["corrected"], has_non_corrected=c["has_non_corrected"], non_corrected=c["non_corrected"],
             bFixScale=c["fix_scale"], min_feat=c["min_feat"], iterations=c["iterations"])
    a.update(kw)
    return pg.Optimizer.OptimizeEssentialGraph(ext, **a)


def _refusals(c):
    ids = c["kf_id"].copy()
    ids[3] = ids[2]
    pose = c["pose"].copy()
    pose["Tcw"][1, 3] = np.nan
    par = c["parent"].copy()
    par[4] = 4
    cor = c["corrected"].copy()
    cor["s"][c["cur_kf"]] = 0.0
    lc = c["loop_conn"].copy()
    lc[0, 1] = c["nkf"]
    selfc = c["loop_conn"].copy()
    selfc[0, 1] = selfc[0, 0]
    cv = c["covis"].copy()
    cv[0] = -1
    pts = c["points"].copy()
    pts["pos"][2, 1] = np.inf
    ref = c["point_ref_kf"].copy()
    ref[0] = c["nkf"]
    return (("kf_id", dict(kf_id=ids)), ("pose", dict(poses=pose)), ("parent", dict(parent=par)), ("scale", dict(corrected=cor)),
            ("loop_conn", dict(loop_conn=lc)), ("self", dict(loop_conn=selfc)), ("covis", dict(covis=cv)), ("point", dict(points=pts)),
            ("ref", dict(point_ref_kf=ref)), ("loop_kf", dict(loop_kf=c["nkf"])), ("cur_kf", dict(cur_kf=-1)), ("iterations", dict(iterations=-1)),
            ("start", dict(covis_start=c["covis_start"][::-1].copy())), ("loop_edge", dict(loop_edge_start=np.arange(c["nkf"] + 1, dtype=np.int32))))


def test_mirror_refuses_malformed_input_without_a_device():
    """Optimizer.OptimizeEssentialGraph raises ValueError for what the library's checked call refuses, before the library is called."""
    c = EC.case("ring12")
    for what, kw in _refusals(c):
        with pytest.raises(ValueError):
            _call(None, c, **kw)
            pytest.fail(what)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=4)
    yield e
    e.close()


def _result(info, poses, sim3, edges, pos):
    ne = int(np.sum(info[3:7]))
    return dict(status=int(info[0]), ret=int(info[2]), iterations=int(info[7]), trials=int(info[8]), free=int(info[2]), vertices=int(info[1]),
                kinds=[int(x) for x in info[3:7]], edges=[(int(e["i"]), int(e["j"]), int(e["kind"])) for e in edges[:ne]], Tcw=poses["Tcw"], Ow=poses["Ow"],
                pos=pos, sim3=np.concatenate([sim3["r"], sim3["t"], sim3["s"][:, None]], 1), chi2=edges["chi2"][:ne], envelope=int(info[9]))


def run_host(ext, c, **kw):
    r = _call(ext, c, **kw)
    info = np.array([r["status"], r["vertices"], r["free"]] + r["kinds"] + [r["iterations"], r["trials"], r["envelope"]], np.int32)
    out = _result(info, r["poses"], r["sim3"], r["edges"], r["points"]["pos"])
    out["ret"] = r["ret"]
    out["bytes"] = (r["poses"].tobytes(), r["sim3"].tobytes(), r["edges"].tobytes(), r["points"].tobytes(), info.tobytes())
    return out


def run_device(ext, c, stream=None, refresh=None, overrides=None):
    """The device form on resident tensors; refresh = (d_kps, d_n, cap, obs arrays): chains pgorb_refresh_map_points_batch_device."""
    import torch
    import pilotguru_amd as pg
    c = dict(c, **(overrides or {}))
    dev = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1).copy()).cuda()
    st = torch.cuda.Stream() if stream == "second" else torch.cuda.current_stream()
    d_pts = dev(c["points"])
    d_pose = dev(c["pose"])
    with torch.cuda.stream(st):
        out = pg.Optimizer.OptimizeEssentialGraph_device(
            ext, torch.from_numpy(c["kf_id"].astype(np.int64)).cuda(), d_pose, c["loop_kf"], c["cur_kf"], i32(c["parent"]), i32(c["loop_conn"]),
            i32(c["loop_edge_start"]), i32(c["loop_edge"]), i32(c["covis_start"]), i32(c["covis"]), i32(c["covis_weight"]), len(c["points"]), d_pts,
            i32(c["point_ref_kf"]), d_kf_bad=dev(c["kf_bad"]), d_point_bad=dev(c["point_bad"]), d_has_corrected=dev(c["has_corrected"]),
            d_corrected=dev(c["corrected"]), d_has_non_corrected=dev(c["has_non_corrected"]), d_non_corrected=dev(c["non_corrected"]),
            bFixScale=c["fix_scale"], min_feat=c["min_feat"], iterations=c["iterations"], stream=st.cuda_stream)
        if refresh is not None:
            kps, n, cap, os_, of, oi = refresh
            nf, npts = c["nkf"], len(c["points"])
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            # (every tensor is named: a temporary would be freed, and its block reused, before the launch reads it)
            hold = [dev(kps), z((nf, cap, 32), torch.uint8), i32(n), dev(c["kf_bad"]), z((npts, 32), torch.uint8), dev(c["point_bad"]), i32(os_), i32(of),
                    i32(oi), z(npts, torch.int32), z(npts, torch.int32)]
            q = lambda t: C.c_void_p(t.data_ptr())
            ext._check(ext._L.pgorb_refresh_map_points_batch_device(
                ext._h, q(hold[0]), q(hold[1]), q(hold[2]), nf, cap, q(out["pose_out"]), q(hold[3]), npts, q(d_pts), q(hold[4]), q(hold[5]), q(hold[6]),
                q(hold[7]), q(hold[8]), len(of), q(hold[9]), npts, None, pg.MP_NORMAL_DEPTH, None, q(hold[10]), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    info = out["info"].cpu().numpy()
    ne = int(info[3:7].sum())
    poses = np.frombuffer(out["pose_out"].cpu().numpy().tobytes(), pg.KF_POSE_DTYPE)
    sim3 = np.frombuffer(out["sim3_out"].cpu().numpy().tobytes(), pg.SIM3D_DTYPE)
    edges = np.frombuffer(out["edge_out"].cpu().numpy().tobytes(), pg.EG_EDGE_DTYPE)[:ne]
    table = np.frombuffer(d_pts.cpu().numpy().tobytes(), pg.MAP_POINT_DTYPE)
    r = _result(info, poses, sim3, edges, table["pos"])
    r["bytes"] = (poses.tobytes(), sim3.tobytes(), edges.tobytes(), table.tobytes(), info.tobytes())
    r["table"] = table
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.NAMES)
def test_gpu_both_forms_equal_the_reference_and_each_other(ext, name):
    c = EC.case(name)
    host = run_host(ext, c)
    bad, seen = EC.compare(name, host)
    bd = EC.bounds(name)
    print("%s: " % name + ", ".join("%s %.3g / %.3g" % (k, seen.get(k, 0.0), bd[k]) for k in EC.FLOAT_OUTPUTS + EC.DOUBLE_OUTPUTS))
    assert bad == [], (name, bad)
    assert host["ret"] == EC.reference(name)["ret"]
    if host["status"] == 0:
        # whatever the arithmetic (the graph without a gauge included): Levenberg keeps a step only if chi2 fell, so the final chi2
        # cannot exceed the chi2 at the input estimates, which no optimisation step has touched
        start = ER.optimize_essential_graph(dict(c, iterations=0))["chi2"]
        assert np.sum(host["chi2"]) <= np.sum(start) * (1 + 1e-9), name
    device = run_device(ext, c)
    assert EC.compare(name, device)[0] == [], name
    assert device["bytes"] == host["bytes"], "%s: the single call equals the device form byte for byte" % name
    other = np.asarray(c["points"]).copy()
    other["pos"] = device["table"]["pos"]
    assert other.tobytes() == device["table"].tobytes(), "normal and distances keep their bytes"
    for p in np.flatnonzero((c["point_bad"] != 0) | (c["point_ref_kf"] < 0) | (c["kf_bad"][np.maximum(c["point_ref_kf"], 0)] != 0)):
        assert device["table"]["pos"][p].tobytes() == c["points"]["pos"][p].tobytes(), "a bad point, no or a bad reference key frame: untouched"
    for i in np.flatnonzero(c["kf_bad"]):
        assert host["Tcw"][i].tobytes() == c["pose"]["Tcw"][i].tobytes() and not host["sim3"][i].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.NAMES)
def test_gpu_repeat_second_stream_and_a_context_that_ran_lba_give_the_same_bytes(ext, name):
    import lba_cases as LC
    c = EC.case(name)
    first = run_device(ext, c)
    assert run_device(ext, c)["bytes"] == first["bytes"], "a repeat"
    assert run_device(ext, c, stream="second")["bytes"] == first["bytes"], "a second stream"
    P, rounds = LC.case("kf2")
    assert not isinstance(LC.run_gpu(P, rounds, ext), int)                  # the same scratch arena, another optimiser's records
    assert run_device(ext, c)["bytes"] == first["bytes"], "after LBA in the same context"
    assert run_host(ext, c)["bytes"] == first["bytes"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.NAMES)
def test_gpu_chain_into_the_map_point_refresh_on_resident_arrays(ext, name):
    """The essential graph -> pgorb_refresh_map_points_batch_device (normal and depth, every point) with nothing downloaded in
    between, against UpdateNormalAndDepth (tests/map_point_reference.py) on the positions and poses the optimiser left.  Every
    point is seen by its reference key frame and by the next one (a bad one in the cases that have one)."""
    import pilotguru_amd as pg
    c = EC.case(name)
    nf, npts, cap = c["nkf"], len(c["points"]), 8
    kps = np.zeros((nf, cap), pg.KEYPOINT_DTYPE)
    kps["octave"] = (np.arange(nf * cap).reshape(nf, cap) * 3) % 8
    kps["x"], kps["y"] = 100.0, 120.0
    ref = c["point_ref_kf"]
    obs = [[(int(ref[p]), p % cap), ((int(ref[p]) + 1) % nf, (p + 3) % cap)] if ref[p] >= 0 else [] for p in range(npts)]
    os_ = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    of, oi = np.array([x[0] for o in obs for x in o], np.int32), np.array([x[1] for o in obs for x in o], np.int32)
    got = run_device(ext, c, refresh=(kps, np.full(nf, cap, np.int32), cap, os_, of, oi))
    assert EC.compare(name, got)[0] == []
    sf = np.asarray(ext.GetScaleFactors(), f32)
    kfs = [MR.KeyFrame(kps[f], np.zeros((cap, 32), np.uint8), got["Ow"][f], bad=c["kf_bad"][f]) for f in range(nf)]
    done = 0
    for p in range(npts):
        row = got["table"][p]
        mp = MR.MapPoint(got["pos"][p], np.zeros(32, np.uint8), bad=bool(c["point_bad"][p]))
        mp.obs = [(kfs[f], i) for f, i in obs[p]]
        mp.ref = kfs[obs[p][0][0]] if obs[p] else None
        if not obs[p] or not MR.update_normal_and_depth(mp, sf, 8):      # a bad point, no observation: the refresh leaves the record alone
            assert row.tobytes() == np.asarray(c["points"])[p].tobytes() or (row["pos"].tobytes() == got["pos"][p].tobytes() and
                                                                           row["normal"].tobytes() == c["points"]["normal"][p].tobytes()), p
            continue
        assert row["normal"].tobytes() == mp.normal.tobytes() and f32(row["min_distance"]) == mp.min_d and f32(row["max_distance"]) == mp.max_d, p
        done += 1
    assert done >= 3 * (nf - int(c["kf_bad"].sum()))


@pytest.mark.gpu
def test_gpu_nothing_and_nonfinite_leave_the_outputs_equal_to_the_inputs(ext):
    import pilotguru_amd as pg
    c = EC.case("nothing")
    for r in (run_host(ext, c), run_device(ext, c)):
        assert r["status"] == pg.EG_NOTHING and r["ret"] == 0 and r["edges"] == [] and r["iterations"] == 0
        assert r["Tcw"].tobytes() == c["pose"]["Tcw"].tobytes() and r["Ow"].tobytes() == c["pose"]["Ow"].tobytes()
        assert r["pos"].tobytes() == c["points"]["pos"].tobytes()
    c = EC.case("ring12")
    cor = c["corrected"].copy()
    cor["t"][c["cur_kf"], 1] = np.nan                         # the checked call refuses it; the device form meets it
    with pytest.raises(ValueError):
        _call(ext, c, corrected=cor)
    r = run_device(ext, c, overrides=dict(corrected=cor))
    want = ER.optimize_essential_graph(dict(c, corrected=cor))
    assert want["status"] == ER.EG_NONFINITE
    assert r["status"] == pg.EG_NONFINITE and r["ret"] == 0 and r["iterations"] == 0 and r["trials"] == 0 and r["edges"] == want["edges"]
    assert r["Tcw"].tobytes() == c["pose"]["Tcw"].tobytes() and r["Ow"].tobytes() == c["pose"]["Ow"].tobytes()
    assert r["table"].tobytes() == np.asarray(c["points"]).tobytes(), "the points are untouched"
    ok = np.arange(c["nkf"]) != c["cur_kf"]
    assert np.array_equal(r["sim3"][ok], want["sim3"][ok]), "sim3_out is the input estimate"


@pytest.mark.gpu
def test_gpu_library_refuses_what_the_mirror_refuses(ext):
    """Each refusal again, past the mirror: the library's own host-side check answers PGORB_E_ARG."""
    import pilotguru_amd as pg
    from pilotguru_amd import _lib
    c = EC.case("ring12")
    p = lambda x: C.c_void_p(x.ctypes.data)
    for what, kw in _refusals(c):
        a = dict(c, **{dict(poses="pose").get(k, k): v for k, v in kw.items()})
        keep = [np.ascontiguousarray(a[k]) for k in ("kf_id", "pose", "kf_bad", "has_corrected", "corrected", "has_non_corrected", "non_corrected",
                                                     "loop_conn", "parent", "loop_edge_start", "covis_start", "covis", "covis_weight", "point_bad",
                                                     "point_ref_kf")]
        le = np.zeros(64, np.int32)                               # (the malformed start array of "loop_edge" names 12 entries)
        pts = np.array(a["points"])
        so, po, eo = np.zeros(c["nkf"], pg.SIM3D_DTYPE), np.zeros(c["nkf"], pg.KF_POSE_DTYPE), np.zeros(4096, pg.EG_EDGE_DTYPE)
        info = np.zeros(pg.EG_INFO, np.int32)
        rc = ext._L.pgorb_optimize_essential_graph(
            ext._h, c["nkf"], p(keep[0]), p(keep[1]), p(keep[2]), int(a["loop_kf"]), int(a["cur_kf"]), 0, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]),
            len(keep[7]), p(keep[7]), p(keep[8]), p(keep[9]), p(le), p(keep[10]), p(keep[11]), p(keep[12]), 100, int(a["iterations"]), len(pts), p(pts),
            p(keep[13]), p(keep[14]), p(so), p(po), p(eo), p(info))
        assert rc == _lib.PGORB_E_ARG, (what, rc)
        assert b"pgorb_optimize_essential_graph" in ext._L.pgorb_last_error(ext._h)


_base = {}


def _chain(n, extra_covis=0, envelope=0):
    """A chain of n key frames whose measurements are made from its vertices (no Sim3 maps), one iteration: n - 1 spanning edges;
    extra_covis rejected covisibles (weight 50) pad the candidates; envelope = the envelope blocks to reach through previous loop
    edges of span 64 (65 rows reach a column: one more than the panel k_eg_step keeps in LDS)."""
    if n not in _base:
        _base[n] = EC.build(n, 5, covis_back=0, loop_conn=np.zeros((0, 3), np.int32), no_maps=True, iterations=1)
    c = dict(_base[n])
    cv = [[] for _ in range(n)]
    for k in range(extra_covis):
        cv[k % n].append(((k % n + 1 + k // n) % n, 50))
    le = [[] for _ in range(n)]
    if envelope:
        need = envelope - (1 + 2 * (n - 2))                   # the chain's own envelope over the n - 1 free vertices
        i = n - 1
        while need > 0 and i > 2:
            span = min(64, i - 2, need)                       # a loop edge from i to i - span - 1 adds span blocks to row i
            le[i].append(i - span - 1)
            need -= span
            i -= 1
        assert need == 0
    c["loop_edge_start"], flat = EC._csr(le)
    c["loop_edge"] = np.asarray(flat, np.int32)
    c["covis_start"], flat = EC._csr(cv)
    c["covis"], c["covis_weight"] = np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.int32)
    return c


@pytest.mark.gpu
def test_gpu_capacities_at_the_limit_and_one_past(ext):
    import pilotguru_amd as pg
    from pilotguru_amd._lib import PGORB_E_LIMIT, PgorbError
    n = pg.EG_MAX_KF
    c = _chain(n, extra_covis=pg.EG_MAX_EDGES - n)            # both capacities at once: 2048 key frames, 65536 candidates
    assert len(c["covis"]) + n == pg.EG_MAX_EDGES
    r = run_host(ext, c)
    assert (r["status"], r["vertices"], r["free"], r["kinds"], r["envelope"]) == (0, n, n - 1, [0, n - 1, 0, 0], 1 + 2 * (n - 2))
    assert _pose_close(r, c, depth=np.arange(n))
    for what, c1 in (("key frames", _chain(n + 1)), ("candidate edges", _chain(n, extra_covis=pg.EG_MAX_EDGES - n + 1))):
        with pytest.raises(PgorbError) as e:
            run_host(ext, c1)
        assert e.value.code == PGORB_E_LIMIT and what in str(e.value), what
        with pytest.raises(PgorbError) as e:
            run_device(ext, c1)
        assert e.value.code == PGORB_E_LIMIT
    c = _chain(n, envelope=pg.EG_MAX_ENVELOPE_BLOCKS)
    r = run_device(ext, c)
    assert (r["status"], r["free"], r["envelope"]) == (0, n - 1, pg.EG_MAX_ENVELOPE_BLOCKS) and r["kinds"][2] > 64
    assert _pose_close(r, c, depth=np.arange(n))
    c1 = _chain(n, envelope=pg.EG_MAX_ENVELOPE_BLOCKS + 1)
    r = run_device(ext, c1)
    assert r["status"] == pg.EG_LIMIT and r["envelope"] == pg.EG_MAX_ENVELOPE_BLOCKS + 1 and r["ret"] == 0 and r["iterations"] == 0
    assert r["Tcw"].tobytes() == c1["pose"]["Tcw"].tobytes() and r["table"].tobytes() == np.asarray(c1["points"]).tobytes()
    with pytest.raises(PgorbError) as e:
        run_host(ext, c1)
    assert e.value.code == PGORB_E_LIMIT and "envelope" in str(e.value)
