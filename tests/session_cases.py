"""Schedules for ONE long-lived context (tests/test_context_session.py): ordered steps (name, family, case, form, stream) over the
families the SLAM loop calls -- extract and match, the projection searches and SearchByBoW, SearchForTriangulation,
CreateNewMapPoints, Fuse, the map-point refresh, the vocabulary -- that share the context's arenas (pgorb_ctx.h: stageA, the
page-locked buffer, stageSfi, stageOut, xdesc, outBlk and the plan arenas, vocab), the captured extract graph and the scratch
ordering across caller streams.

No reference is written here: every step's expected result comes from its family's pinned reference (matcher_reference,
triangulation_reference, mapping_reference, fuse_reference, map_point_reference, vocab_reference, oracle.OrbOracle and
oracle.hamming_best2), computed on the CPU and cached per (family, case).  Every comparison is exact.

A step declares the EDGES it is there for, the arenas it must reallocate (`grow`) and the arenas it must leave where they are
(`still`); the runner reads the arenas through pgorb_debug_arena before and after the step and asserts both.  What "large" means
is derived from the request sizes: ensure() rounds a request up to 4 KiB and grows only past that, pg_ctx_pinned() keeps 25 %
head-room, so a growing step asks for more than 1.25 x (+ 4 KiB) of what the context has seen -- sizes() below computes the
requests the schedules rely on.
"""
import collections
import contextlib
import functools
import os
import sys
import tempfile
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_cases as FC  # noqa: E402
import fuse_reference as FR  # noqa: E402
import map_point_cases as PC  # noqa: E402
import map_point_reference as MPR  # noqa: E402
import mapping_cases as MC  # noqa: E402
import matcher_cases as MA  # noqa: E402
import triangulation_cases as TC  # noqa: E402
import vocab_cases as VC  # noqa: E402
import vocab_reference as VR  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE  # noqa: E402
from pilotguru_amd.synth import synth_ride  # noqa: E402

NFEATURES = 1000
ARENAS = ("stageA", "pinned", "stageSfi", "stageOut", "xdesc", "outBlk", "plan_pyr", "vocab")          # plan_pyr stands for the plan arenas

# what the schedules must cover: every shared arena, and every item of sections (a)-(f) of the session test
EDGES = ["arena_stageA", "arena_pinned", "arena_stageSfi", "arena_stageOut", "arena_xdesc", "arena_outBlk", "arena_plan", "arena_vocab",
         "a_fuse_rounds_refresh_projection", "a_bow_after_triangulation", "a_best2_match_batch_best2", "a_vocab_swap",
         "a_host_after_device", "a_device_after_host",
         "b_direct_capture_replay", "b_pinned_reallocated", "b_frame_size_and_back", "b_nframes", "b_pipeline_levels",
         "b_cond_nframes", "b_cond_epoch", "b_cond_pinned", "b_cond_outbytes",
         "c_streams_a_b_a", "c_null_stream",
         "d_frame_stream", "d_device_frame_stream", "d_match_mode_0_after_stream",
         "e_two_contexts", "e_options_differ", "e_vocabularies_differ",
         "f_destroy_with_queued_work"]

Step = collections.namedtuple("Step", "name family case form stream ctx edges grow still")


def step(name, family, case, form="host", stream=None, ctx=0, edges=(), grow=(), still=()):
    return Step(name, family, case, form, stream, ctx, tuple(edges), tuple(grow), tuple(still))


FORMS = {"extract": ("host", "device"), "best2": ("host",), "match_batch": ("device",), "hmatrix": ("host",),
         "matcher": ("host", "device"), "triangulation": ("host", "device"), "mapping": ("host", "device"), "fuse": ("host", "device"),
         "fuse_rounds": ("host",), "refresh": ("host", "device"), "vocab_upload": ("host", "device"), "bow_transform": ("host", "device"),
         "option": ("host",)}
CHECKED = [f for f in FORMS if f not in ("vocab_upload", "option")]           # families whose step returns a result to compare


# outBlk holds max_batch x (the sum over levels of max(quota + 2, 4 x roots)) keypoints, whatever the frame size: with 1000 features
# the quotas always win and the block never grows.  The schedules that must see it grow run on a context of 40 features and 2 levels
# (quotas 22 and 18): 160 x 120 has one root per level (24 + 20 slots), 640 x 80 has eight (32 + 32).
FEW = "@40,2"
CONTEXT = {"a_plan": dict(nfeatures=40, nlevels=2), "b": dict(nfeatures=40, nlevels=2)}


def make_context(pg, batch=4, nfeatures=NFEATURES, nlevels=MC.NLEVELS):
    return pg.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, max_width=640, max_height=480, max_batch=batch)


# ---------------------------------------------------------------- cases, by family and name
@functools.lru_cache(None)
def _matcher_index():
    return {c["name"]: c for c in MA.all_cases()}


@functools.lru_cache(None)
def _tri_index():
    return {c["name"]: c for c in TC.all_cases()}


@functools.lru_cache(None)
def _fuse_index():
    return {c.name: c for c in FC.edge_cases()}


@functools.lru_cache(None)
def _refresh_index():
    return {c.name: c for c in PC.edge_cases()}


@functools.lru_cache(None)
def _vocab_index():
    return {c.tree.name: c for c in VC.all_cases()}


@functools.lru_cache(None)
def _vocab_dir():
    return tempfile.mkdtemp(prefix="pgorb_session_")


# groups of constructed cases that one batched launch can take (same scalar parameters), each with a match AND a query without one
MATCHER_GROUPS = {
    "sfi_hist": ("count_ties_sfi", "half_bins_sfi"), "sfi_second": ("count_ties_second_sfi", "tenth_below_max3_sfi"),
    "frame_hist": ("count_ties_frame", "half_bins_frame"), "frame_second": ("count_ties_second_frame", "tenth_below_max2_frame"),
    "frame_many": ("tenth_equal_max3_frame", "count_ties_frame"),
    "frame_dense": ("overlapping_dense_queries_frame", "tie_at_400_frame", "tie_at_321_frame", "occupied_best_frame"),
    "keyframe_hist": ("count_ties_keyframe", "half_bins_keyframe"),
    "points_small": ("occupied_best_points",), "points_ties": ("tie_at_400_points", "tie_at_320_points", "occupied_best_points"),
    "bow_hist": ("count_ties_bow", "half_bins_bow"), "bow_ties": ("count_ties_bow",), "bow_half": ("half_bins_bow",),
}
TRI_GROUPS = {
    "ties": ("equal distances: the later passing one wins", "two KF1 keypoints share one KF2 keypoint", "has_point1 skips"),
    "nodes": ("node with 300 KF2 keypoints", "0.1 rule: 11 and 1 dropped", "tie across register slots (positions 70, 190)"),
    "rotation": ("0.1 rule: 11 and 1 dropped", "rotation bin 30 -> 0", "dist 51 never kept"),
}
FUSE_GROUPS = {"chains": ("chain3_overlap", "chain2_bad", "dist_51", "tie"), "depth": ("depth_min", "depth_max_past", "octave_above"),
               "reading": ("reading_gemm", "reading_dot", "chain1_live_more")}
REFRESH_GROUPS = {"shared": ("shared_key_frames",), "lengths": ("n63", "n64", "n65", "bad_point", "equal_medians"),
                  "selection": ("selection_skips", "n4_median_index_1", "all_kf_bad")}
MAPPING_SCENES = {"scene1": dict(seed=1), "scene2_small": dict(seed=2, nneigh=3, npts=120), "scene3_small": dict(seed=3, nneigh=2, npts=150)}
VOCABS = {"ragged": "ragged1", "random": "random1_k10_L6"}


def _group(families, index, name):
    return [index()[n] for n in families[name]]


@functools.lru_cache(None)
def _frames(case):
    """'WxHxN:seed[@nfeatures,nlevels]' -> N frames"""
    size, seed = case.split("@")[0].split(":")
    w, h, n = (int(x) for x in size.split("x"))
    return synth_ride(int(seed), w, h, n)


def _extractor_of(case):
    nf, nl = (int(x) for x in case.split("@")[1].split(",")) if "@" in case else (NFEATURES, MC.NLEVELS)
    return nf, 1.2, nl


@functools.lru_cache(None)
def _hamming(case):
    """'NAxNB:seed' (best2, hmatrix) -> (a, b) with exact duplicates planted; 'BxCAPxP:seed' (match_batch) -> desc, counts, pairs"""
    size, seed = case.split(":")
    dims = [int(x) for x in size.split("x")]
    rng = np.random.RandomState(int(seed))
    if len(dims) == 2:
        na, nb = dims
        a, b = rng.randint(0, 256, (na, 32)).astype(np.uint8), rng.randint(0, 256, (nb, 32)).astype(np.uint8)
        k = min(na, nb) // 4
        b[rng.choice(nb, k, replace=False)] = a[rng.choice(na, k, replace=False)]
        return a, b
    B, cap, P = dims
    desc = rng.randint(0, 256, (B, cap, 32)).astype(np.uint8)
    counts = [cap - 3 * f for f in range(B)]
    for f in range(1, B):
        desc[f, :counts[f]:3] = desc[f - 1, :counts[f]:3]
    return desc, counts, [((f + 1) % B, f) for f in range(P)]


@functools.lru_cache(None)
def _vocab_case(name):
    idx = _vocab_index()
    c = idx[VOCABS[name]]
    path = VC.write_text(c.tree, os.path.join(_vocab_dir(), name + ".txt"))
    return c, path


@functools.lru_cache(None)
def _neighbourhood_tail():
    """The refresh that ends SearchInNeighbors on FC.neighbourhood(5, ...): the case built from the REFERENCE's map after both Fuse
    rounds (tests/test_map_point_refresh.py builds the same one), and what the rounds return."""
    from test_map_point_refresh import _refresh_objects
    cur, targets, points = FC.neighbourhood(5, 640, 480, 20, 1000, 500.0)
    want_n = FR.search_in_neighbors(cur, targets)
    live = [mp for mp in cur.slots if mp is not None and not mp.bad]
    live = list({mp.id: mp for mp in live}.values())
    return _refresh_objects([cur] + targets, live), want_n, FC.map_state([cur] + targets, points)


def refresh_cases(name):
    return [_neighbourhood_tail()[0]] if name == "neighbourhood_tail" else _group(REFRESH_GROUPS, _refresh_index, name)


# ---------------------------------------------------------------- the reference result of a step, and whether it says anything
@functools.lru_cache(None)
def reference(family, case, oracle=None):
    if family == "extract":
        ora = oracle.OrbOracle(*_extractor_of(case), 20, 7)
        return [ora.extract(f) for f in _frames(case)]
    if family == "best2":
        return oracle.hamming_best2(*_hamming(case))
    if family == "match_batch":
        desc, counts, pairs = _hamming(case)
        return [oracle.hamming_best2(desc[q, :counts[q]], desc[t, :counts[t]]) for q, t in pairs]
    if family == "hmatrix":
        a, b = _hamming(case)
        return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2).astype(np.uint16)         # popcount of the XOR, nothing to restate
    if family == "matcher":
        return [MA.run_reference(c) for c in _group(MATCHER_GROUPS, _matcher_index, case)]
    if family == "triangulation":
        return [TC.run_reference(c) for c in _group(TRI_GROUPS, _tri_index, case)]
    if family == "mapping":
        return MC.run_reference(*MC.scene(**MAPPING_SCENES[case]))
    if family == "fuse":
        return [FC.run_reference(c) for c in _group(FUSE_GROUPS, _fuse_index, case)]
    if family == "fuse_rounds":
        return _neighbourhood_tail()[1:]
    if family == "refresh":
        return [PC.run_reference(c) for c in refresh_cases(case)]
    if family == "bow_transform":
        name, lu = case.split(":")
        c, path = _vocab_case(name)
        return VR.Vocabulary.load_text(path).transform_features(c.queries, int(lu))
    return None


def nontrivial(family, case, ref):
    """A result that stale data of the step before could not pass for: something found, and (matchers) something not found."""
    if family == "extract":
        return all(len(k) > min(100, _extractor_of(case)[0] // 2) for k, _ in ref)
    if family == "best2":                   # nearest neighbour always answers: planted duplicates (0) beside ordinary distances
        return bool((ref[1] == 0).any() and (ref[1] > 0).any() and len(set(ref[0].tolist())) > 10)
    if family == "match_batch":
        return all((r[1] == 0).any() and (r[1] > 0).any() for r in ref)
    if family == "hmatrix":
        return bool((ref == 0).any() and len(np.unique(ref)) > 10)
    if family == "matcher":
        cs = _group(MATCHER_GROUPS, _matcher_index, case)
        found = sum(int((np.asarray(r[1]) >= 0).sum()) for r in ref)
        asked = sum(len(c["a"]["valid"]) if "valid" in c["a"] else len(np.asarray(r[1])) for c, r in zip(cs, ref))
        return found >= 1 and found < asked
    if family == "triangulation":
        return sum(int(r[0]) for r in ref) >= 1 and any((np.asarray(r[1]) < 0).any() for r in ref)
    if family == "mapping":
        return len(ref[0]) >= 1
    if family == "fuse":
        return sum(int(r[0]) for r in ref) >= 1 and any((r[1] != r[1][0]).any() or int(r[0]) == 0 for r in ref)
    if family == "fuse_rounds":
        return sum(ref[0]) >= 1
    if family == "refresh":
        return any((r[3] == 3).any() for r in ref)
    if family == "bow_transform":
        return bool((ref[1] > 0).any() and len(set(ref[0].tolist())) > 1)
    return True


# ---------------------------------------------------------------- running a step on a context
def _stream_ptr():
    import ctypes as C
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(st, ext):
    """The step's result from the GPU, in the shape reference() returns.  Device forms run on torch's current stream."""
    import ctypes as C
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd import vocab as V
    fam, case, dev = st.family, st.case, st.form == "device"
    if fam == "option":
        ext.set_option(*case)
        return None
    if fam == "extract":
        fr = _frames(case)
        if not dev:
            return ext.extract_batch(list(fr))
        kps, desc, n = ext.extract_batch_device(torch.from_numpy(fr).cuda())
        torch.cuda.synchronize()
        n = n.cpu().numpy()
        kh = kps.cpu().numpy().view(np.uint8).reshape(len(fr), -1, 28)
        return [(kh[f, :n[f]].copy().view(KEYPOINT_DTYPE).reshape(-1), desc[f, :n[f]].cpu().numpy()) for f in range(len(fr))]
    if fam == "best2":
        return ext.hamming_best2(*_hamming(case))
    if fam == "hmatrix":
        return ext.hamming_matrix(*_hamming(case))
    if fam == "match_batch":
        desc, counts, pairs = _hamming(case)
        d, n = torch.from_numpy(desc).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda")
        pq = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
        pt = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
        bi, b1, b2 = ext.match_batch_device(d, n, pq, pt)
        torch.cuda.synchronize()
        return [(bi[k, :counts[q]].cpu().numpy(), b1[k, :counts[q]].cpu().numpy().view(np.uint16), b2[k, :counts[q]].cpu().numpy().view(np.uint16))
                for k, (q, _) in enumerate(pairs)]
    if fam == "matcher":
        cs = _group(MATCHER_GROUPS, _matcher_index, case)
        return MA.run_gpu_batched(cs, ext, "nan")[1] if dev else [MA.run_gpu(c, ext) for c in cs]
    if fam == "triangulation":
        cs = _group(TRI_GROUPS, _tri_index, case)
        return TC.run_gpu_batched(cs, ext)[0] if dev else [TC.run_gpu(c, ext) for c in cs]
    if fam == "mapping":
        KF1, neigh = MC.scene(**MAPPING_SCENES[case])
        return MC.run_gpu_batched([(KF1, neigh)], ext)[0][:5] if dev else MC.run_gpu(KF1, neigh, ext)
    if fam == "fuse":
        cs = _group(FUSE_GROUPS, _fuse_index, case)
        return [g[:5] for g in FC.run_gpu_batched(cs, ext)] if dev else [FC.run_gpu(c, ext) for c in cs]
    if fam == "fuse_rounds":
        cur, targets, points = FC.neighbourhood(5, 640, 480, 20, 1000, 500.0)
        return FC.search_in_neighbors_gpu(ext, cur, targets, points), FC.map_state([cur] + targets, points)
    if fam == "refresh":
        cs = refresh_cases(case)
        if dev:
            out, untouched = PC.run_gpu_batched(cs, ext, MPR.BOTH)
            assert untouched, "%s wrote past nsel or outside the selected points" % st.name
            return out
        return [PC.run_gpu(c, ext) for c in cs]
    if fam == "vocab_upload":
        voc = V.ORBVocabulary(text_file=_vocab_case(case)[1])
        if dev:
            t = torch.from_numpy(voc.blob()).cuda()
            ext._check(ext._L.pgorb_vocab_upload_device(ext._h, C.c_void_p(t.data_ptr()), t.numel(), _stream_ptr()))
            torch.cuda.synchronize()
        else:
            voc.upload(ext)
        return None
    if fam == "bow_transform":
        name, lu = case.split(":")
        q = np.ascontiguousarray(_vocab_case(name)[0].queries, np.uint8)
        n = len(q)
        if dev:
            d = torch.from_numpy(q).cuda()
            word, node = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
            weight = torch.zeros(n, dtype=torch.float64, device="cuda")
            p = lambda t: C.c_void_p(t.data_ptr())
            ext._check(ext._L.pgorb_bow_transform_device(ext._h, p(d), n, int(lu), p(word), p(weight), p(node), _stream_ptr()))
            torch.cuda.synchronize()
            return word.cpu().numpy().view(np.uint32), weight.cpu().numpy(), node.cpu().numpy().view(np.uint32)
        word, node, weight = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
        p = lambda a: C.c_void_p(a.ctypes.data)
        ext._check(ext._L.pgorb_bow_transform(ext._h, p(q), n, int(lu), p(word), p(weight), p(node)))
        return word, weight, node
    raise ValueError(fam)


def _bytes(x):
    """A result as nested tuples of bytes and ints: equal results have equal images"""
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return tuple(_bytes(v) for v in x)
    if isinstance(x, np.ndarray):
        return (x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return np.float32(x).tobytes()
    return x


def same(family, want, got):
    if family == "matcher":
        return MA.same(want, got)
    if family == "triangulation":
        return len(want) == len(got) and all(TC.same(w, g) for w, g in zip(want, got))
    if family == "mapping":
        return (MC.same_point_lists(want[0], got[0]) and [int(x) for x in want[1]] == [int(x) for x in got[1]] and
                all(np.asarray(w, np.float32).tobytes() == np.asarray(g, np.float32).tobytes() for w, g in zip(want[2:4], got[2:4])) and
                np.array_equal(np.asarray(want[4]), np.asarray(got[4])))
    if family == "fuse":
        return len(want) == len(got) and all(FC.same(w, g) for w, g in zip(want, got))
    if family == "fuse_rounds":
        return list(want[0]) == list(got[0]) and want[1] == got[1]
    if family == "refresh":
        return len(want) == len(got) and all(PC.same(w, g) for w, g in zip(want, got))
    if family == "extract":
        return len(want) == len(got) and all(wk.tobytes() == gk.tobytes() and np.array_equal(wd, gd) for (wk, wd), (gk, gd) in zip(want, got))
    return _bytes(want) == _bytes(got)


def arenas(ext):
    return {a: ext.debug_arena(a) for a in ARENAS}


class Session:
    """Runs steps on its contexts one after the other; after every step: synchronise, pgorb_check_async, compare with the reference,
    and check the arenas the step declared.  Failures name the step, its index and the step before it."""

    def __init__(self, contexts, oracle):
        self.ctx, self.oracle, self.index, self.prev, self.log = contexts, oracle, 0, None, []

    def where(self, st):
        return "step %d '%s' (%s %s, %s form) after '%s'" % (self.index, st.name, st.family, st.case, st.form, self.prev)

    def check(self, st, got):
        if st.family in CHECKED:
            want = reference(st.family, st.case, self.oracle)
            assert same(st.family, want, got), "%s: differs from the reference" % self.where(st)

    def sync(self, st, ext):
        import torch
        try:
            torch.cuda.synchronize()
            ext.check_async()
        except Exception as e:                  # an asynchronous error belongs to the step that has just run
            raise AssertionError("%s: %s" % (self.where(st), e))

    def step(self, st):
        ext = self.ctx[st.ctx]
        before = arenas(ext)
        try:
            got = run(st, ext)
        except AssertionError:
            raise
        except Exception as e:
            raise AssertionError("%s: %s: %s" % (self.where(st), type(e).__name__, e))
        self.sync(st, ext)
        after = arenas(ext)
        self.check(st, got)
        self.log.append((st.name, {a: (before[a], after[a]) for a in ARENAS if before[a] != after[a]}))
        for a in st.grow:
            assert after[a][1] > before[a][1], "%s: was to reallocate %s, which stayed at %r" % (self.where(st), a, before[a])
        for a in st.still:
            assert after[a] == before[a], "%s: was to leave %s alone: %r -> %r" % (self.where(st), a, before[a], after[a])
        self.index, self.prev = self.index + 1, st.name
        return before, after

    def run(self, steps):
        for st in steps:
            self.step(st)


# ---------------------------------------------------------------- work queued without a host synchronisation
class Queued:
    """A step whose *_batch_device runner (the per-family run_gpu_batched, used as it is) is stopped after it has QUEUED its work:
    the runner runs in a helper thread under torch stream `stream` (None: the null stream) and is parked inside the
    torch.cuda.synchronize() that follows its launch; finish() lets it collect.  Only one thread ever runs at a time, so the
    context is never entered concurrently; the host just does not wait between the launches of different steps."""
    _local = threading.local()
    _real = None

    def __init__(self, fn, stream, park_at=1):
        self.fn, self.stream, self.park_at, self.count = fn, stream, park_at, 0
        self.parked, self.go = threading.Semaphore(0), threading.Semaphore(0)
        self.result = self.error = None
        self.thread = threading.Thread(target=self._body)

    def _body(self):
        import torch
        Queued._local.me = self
        try:
            with (torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()):
                self.result = self.fn()
        except BaseException as e:              # handed to finish()
            self.error = e
        finally:
            self.parked.release()

    @staticmethod
    def _synchronize(*a, **k):
        import torch
        me = getattr(Queued._local, "me", None)
        if me is None:
            return Queued._real(*a, **k)
        me.count += 1
        if me.count == me.park_at:
            me.parked.release()
            me.go.acquire()
        torch.cuda.current_stream().synchronize()          # this step's own stream only

    @staticmethod
    @contextlib.contextmanager
    def patched():
        import torch
        Queued._real = torch.cuda.synchronize
        torch.cuda.synchronize = Queued._synchronize
        try:
            yield
        finally:
            torch.cuda.synchronize = Queued._real

    def start(self):
        self.thread.start()
        self.parked.acquire()
        if self.error is not None:
            self.finish()
        return self

    def finish(self):
        self.go.release()
        self.thread.join()
        if self.error is not None:
            raise self.error
        return self.result


PARK_AT = {"matcher": 2}                         # matcher_cases.run_gpu_batched synchronises once after the grid, then after the search


# ---------------------------------------------------------------- the schedules
E320 = ["320x240x1:%d" % s for s in range(31, 40)]
E640 = ["640x480x1:%d" % s for s in range(41, 44)]


def schedule_a():
    """Grow / shrink / regrow of every shared arena: first used by family X at a small size, grown by a different family Y, X
    again (nothing moves), Y again (nothing moves).  Request sizes: see sizes()."""
    S = step
    return [
        # xdesc (match_mode 0: train descriptors as +-1 bytes, 2 KiB per 16 of them and pair): X = hamming_best2, Y = match_batch_device
        S("mode0", "option", ("match_mode", 0)),
        S("best2_small", "best2", "300x400:1", edges=["arena_xdesc", "arena_stageA", "arena_pinned", "a_best2_match_batch_best2"],
          grow=["xdesc", "stageA", "pinned"]),
        S("match_batch_large", "match_batch", "4x2000x3:2", "device", grow=["xdesc"], still=["stageA", "pinned"]),
        S("best2_small_again", "best2", "300x400:1", still=["xdesc", "stageA", "pinned"]),
        S("match_batch_large_again", "match_batch", "4x2000x3:3", "device", still=["xdesc", "stageA", "pinned"]),
        # stageSfi: X = SearchByBoW (one byte per keypoint: 4 KiB), grown by Fuse (40 B per query or keypoint: sizes()) and then by the
        # projection search (candidate lists, 1286 B per query); stageA / pinned: X = best2, Y = Fuse, then the refresh
        S("bow_small", "matcher", "bow_ties", edges=["arena_stageSfi"], grow=["stageSfi"]),
        S("fuse_rounds", "fuse_rounds", "neighbourhood", edges=["a_fuse_rounds_refresh_projection"], grow=["stageA", "pinned", "stageSfi"]),
        S("refresh_tail", "refresh", "neighbourhood_tail", grow=["stageA", "pinned"]),
        S("projection_after_refresh", "matcher", "frame_many", grow=["stageSfi"], still=["stageA", "pinned"]),
        S("bow_small_again", "matcher", "bow_half", still=["stageA", "pinned", "stageSfi"]),
        S("best2_small_third", "best2", "300x400:4", still=["stageA", "pinned", "xdesc"]),
        S("projection_again", "matcher", "frame_hist", still=["stageA", "pinned", "stageSfi"]),
        S("sfi_small", "matcher", "sfi_second", still=["stageA", "pinned", "stageSfi"]),
        S("refresh_tail_again", "refresh", "lengths", still=["stageA", "pinned", "stageSfi"]),
        # bins of two layouts in stageSfi: SearchForTriangulation, then SearchByBoW, in both forms
        S("triangulation_device", "triangulation", "nodes", "device", edges=["a_bow_after_triangulation"]),
        S("bow_device", "matcher", "bow_hist", "device", still=["stageA", "pinned"]),
        S("triangulation_host", "triangulation", "ties", edges=["a_host_after_device"]),
        S("bow_host", "matcher", "bow_ties", edges=["a_host_after_device"]),
        S("bow_device_again", "matcher", "bow_half", "device", edges=["a_device_after_host"]),
        S("triangulation_device_again", "triangulation", "rotation", "device", edges=["a_device_after_host"]),
        # CreateNewMapPoints, Fuse and the refresh: host form directly after the device form of the same family, and the reverse
        S("mapping_device", "mapping", "scene1", "device"),
        S("mapping_host", "mapping", "scene2_small", edges=["a_host_after_device"]),
        S("mapping_device_again", "mapping", "scene3_small", "device", edges=["a_device_after_host"]),
        S("fuse_device", "fuse", "chains", "device"),
        S("fuse_host", "fuse", "depth", edges=["a_host_after_device"]),
        S("fuse_device_again", "fuse", "reading", "device", edges=["a_device_after_host"]),
        S("refresh_device", "refresh", "shared", "device"),
        S("refresh_host", "refresh", "selection", edges=["a_host_after_device"]),
        S("refresh_device_again", "refresh", "lengths", "device", edges=["a_device_after_host"]),
        S("points_after_all", "matcher", "points_ties", "device", still=["stageA", "pinned", "stageSfi"]),
        # stageOut: X = the device upload's validation flag (64 B), Y = the Hamming matrix; vocab: a second, larger vocabulary
        S("vocab_small", "vocab_upload", "ragged", "device", edges=["arena_stageOut", "arena_vocab", "a_vocab_swap"], grow=["stageOut", "vocab"]),
        S("bow_transform_small", "bow_transform", "ragged:0"),
        S("hmatrix_large", "hmatrix", "300x400:5", grow=["stageOut"], still=["vocab"]),
        S("vocab_large", "vocab_upload", "random", "device", grow=["vocab"], still=["stageOut"]),
        S("bow_transform_large", "bow_transform", "random:1", "device"),
        S("hmatrix_large_again", "hmatrix", "300x400:6", still=["stageOut", "vocab"]),
        S("vocab_small_again", "vocab_upload", "ragged", still=["stageOut", "vocab"]),
        S("bow_transform_small_again", "bow_transform", "ragged:1", "device", still=["vocab"]),
        S("vocab_large_again", "vocab_upload", "random", still=["stageOut", "vocab"]),
        S("bow_transform_large_again", "bow_transform", "random:0", still=["vocab"]),
    ]


S160 = ["160x120x1:%d%s" % (s, FEW) for s in range(31, 40)]
WIDE = ["640x80x1:%d%s" % (s, FEW) for s in range(41, 44)]


def schedule_a_plan():
    """outBlk and the plan arenas: X = the host-frame extract at 160 x 120, Y = the device extract at 640 x 80 (more pyramid bytes,
    and eight quadtree roots per level instead of one)."""
    S = step
    return [S("extract_small", "extract", S160[0], edges=["arena_outBlk", "arena_plan"], grow=["outBlk", "plan_pyr"]),
            S("extract_device_large", "extract", "640x80x2:7" + FEW, "device", grow=["outBlk", "plan_pyr"]),
            S("extract_small_again", "extract", S160[1], still=["outBlk", "plan_pyr", "stageA"]),
            S("extract_device_large_again", "extract", "640x80x2:8" + FEW, "device", still=["outBlk", "plan_pyr"])]


def schedule_b():
    """The captured extract graph against what invalidates it.  A step's case carries the expected HostGraph state of its extract:
    (frames, 0 direct | 1 captured | 2 replayed | None = either, decided by where the allocator puts the page-locked buffer)."""
    S = step
    return [
        S("direct", "extract", (S160[0], 0), edges=["b_direct_capture_replay"], grow=["outBlk", "pinned"]),
        S("capture", "extract", (S160[1], 1), still=["outBlk", "pinned"]),
        S("replay", "extract", (S160[2], 2), still=["outBlk", "pinned"]),
        # a host matcher call whose download is larger than the extract's: the page-locked buffer the graph copies into goes away
        S("matcher_download", "best2", "30000x500:9", edges=["b_pinned_reallocated", "b_cond_pinned"], grow=["pinned"], still=["outBlk"]),
        S("after_pinned_moved", "extract", (S160[3], None), still=["pinned"]),
        S("replay_again", "extract", (S160[4], 2), still=["pinned", "outBlk"]),
        # a second frame size and back: new plans (planEpoch), outBlk regrown
        S("other_size", "extract", (WIDE[0], 0), edges=["b_frame_size_and_back", "b_cond_epoch", "b_cond_outbytes"], grow=["outBlk", "plan_pyr"]),
        S("first_size_back", "extract", (S160[5], 0), still=["outBlk", "plan_pyr"]),
        S("first_size_capture", "extract", (S160[6], 1)),
        S("first_size_replay", "extract", (S160[7], 2)),
        # another number of frames
        S("two_frames", "extract", ("160x120x2:51" + FEW, 0), edges=["b_nframes", "b_cond_nframes", "b_cond_outbytes"], still=["outBlk"]),
        S("one_frame_again", "extract", (S160[8], 2)),              # the one-frame graph is still the captured one, and still fits
        S("two_frames_capture", "extract", ("160x120x2:52" + FEW, 1)),
        S("two_frames_replay", "extract", ("160x120x2:53" + FEW, 2)),
        S("one_frame_no_stale_replay", "extract", (S160[0], 0), edges=["b_cond_nframes"]),     # the graph now holds two frames
        # an option that bypasses the graph
        S("pipeline_on", "option", ("pipeline_levels", 4), edges=["b_pipeline_levels", "b_cond_epoch"]),
        S("pipelined", "extract", (S160[1], 0)),
        S("pipelined_again", "extract", (S160[2], 0)),
        S("pipeline_off", "option", ("pipeline_levels", 0)),
        S("off_direct", "extract", (S160[3], 0)),
        S("off_capture", "extract", (S160[4], 1)),
        S("off_replay", "extract", (S160[5], 2)),
    ]


# which declared edge answers for each replay condition of HostGraph (extract.hip): dropping the condition makes the named step
# replay a graph that no longer fits
REPLAY_CONDITIONS = {"G.nframes == nframes": "b_cond_nframes", "G.epoch == c->planEpoch": "b_cond_epoch", "G.pinned == hv": "b_cond_pinned",
                     "G.outBytes == outBytes": "b_cond_outbytes"}


def schedule_c(null_stream):
    """Two caller streams and no host synchronisation in between: the projection search at the schedule's largest case on A, then
    SearchByBoW, Fuse and the refresh on B, then a user on A again.  stream: 'A' | 'B'; with null_stream one of them is stream 0."""
    S = step
    e = ["c_null_stream"] if null_stream else ["c_streams_a_b_a"]
    return [S("projection_on_a", "matcher", "frame_dense", "device", "A", edges=e),
            S("bow_on_b", "matcher", "bow_hist", "device", "B", edges=e),
            S("fuse_on_b", "fuse", "chains", "device", "B", edges=e),
            S("refresh_on_b", "refresh", "shared", "device", "B", edges=e),
            S("points_on_a", "matcher", "points_ties", "device", "A", edges=e)]


def schedule_d():
    """What runs on the context between a stream's submit and its wait: steps that regrow xdesc and stageA."""
    S = step
    return [S("mode0_after_streams", "option", ("match_mode", 0), edges=["d_frame_stream", "d_device_frame_stream", "d_match_mode_0_after_stream"]),
            S("best2_between", "best2", "300x400:1", grow=["stageA"]),
            S("match_batch_between", "match_batch", "4x2000x3:2", "device", grow=["xdesc"]),
            S("refresh_between", "refresh", "neighbourhood_tail", grow=["stageA"])]


def schedule_e():
    """Two contexts alive together, steps alternating: context 0 in match_mode 0 with the small vocabulary, context 1 with the
    defaults and the large one."""
    S = step
    e = ["e_two_contexts"]
    return [S("mode0_on_0", "option", ("match_mode", 0), ctx=0, edges=["e_options_differ"]),
            S("vocab_on_0", "vocab_upload", "ragged", ctx=0, edges=["e_vocabularies_differ"]),
            S("vocab_on_1", "vocab_upload", "random", "device", ctx=1, edges=["e_vocabularies_differ"]),
            S("best2_on_0", "best2", "300x400:1", ctx=0, edges=e), S("best2_on_1", "best2", "300x400:4", ctx=1, edges=e),
            S("bow_transform_on_0", "bow_transform", "ragged:0", ctx=0, edges=e),
            S("bow_transform_on_1", "bow_transform", "random:1", "device", ctx=1, edges=e),
            S("refresh_on_0", "refresh", "shared", "device", ctx=0, edges=e), S("refresh_on_1", "refresh", "lengths", ctx=1, edges=e),
            S("extract_on_0", "extract", E320[0], ctx=0, edges=e), S("extract_on_1", "extract", E640[0], ctx=1, edges=e),
            S("fuse_on_1", "fuse", "chains", "device", ctx=1, edges=e), S("fuse_on_0", "fuse", "depth", ctx=0, edges=e),
            S("bow_transform_again_on_0", "bow_transform", "ragged:1", "device", ctx=0, edges=e),
            S("bow_transform_again_on_1", "bow_transform", "random:0", ctx=1, edges=e),
            S("extract_again_on_0", "extract", E320[1], ctx=0, edges=e), S("extract_again_on_1", "extract", E640[1], ctx=1, edges=e)]


def schedule_f():
    """Context 1 is closed while context 0 has queued, un-waited work on a stream of its own."""
    S = step
    e = ["f_destroy_with_queued_work"]
    return [S("refresh_queued_on_0", "refresh", "shared", "device", "A", ctx=0, edges=e),
            S("fuse_on_1", "fuse", "chains", ctx=1, edges=e),
            S("mapping_queued_on_0", "mapping", "scene2_small", "device", "A", ctx=0, edges=e)]


def plain(st):
    """A step of schedule_b without the expected graph state"""
    return st._replace(case=st.case[0]) if st.family == "extract" and isinstance(st.case, tuple) else st


SCHEDULES = collections.OrderedDict([("a", schedule_a), ("a_plan", schedule_a_plan), ("b", schedule_b), ("c", lambda: schedule_c(False)), ("c_null", lambda: schedule_c(True)),
                                     ("d", schedule_d), ("e", schedule_e), ("f", schedule_f)])


def sizes():
    """The request sizes (bytes) that decide which steps of schedule_a and schedule_b reallocate, from the call's own arithmetic
    (PgHostCall regions are 64-byte aligned; only the dominant regions are counted, so these are lower bounds)."""
    out = {}
    out["best2 300x400: stageA = pinned request"] = 300 * 32 + 400 * 32 + 32 + 300 * 8
    out["best2 300x400: xdesc (2 KiB per 16 train descriptors and pair)"] = 25 * 2048
    out["match_batch 4x2000x3: xdesc"] = 3 * 125 * 2048
    c = _neighbourhood_tail()[0]
    cap = max(len(k) for k, _, _, _ in c.kfs)
    out["refresh of the neighbourhood: stageA = pinned request"] = len(c.kfs) * cap * (28 + 32) + len(c.points) * (44 + 32)
    out["best2 30000x500: download"] = 30000 * 8
    out["SearchByBoW, 22 keypoints: stageSfi (a byte per keypoint)"] = 22 + 256
    cur, targets, points = FC.neighbourhood(5, 640, 480, 20, 1000, 500.0)
    out["Fuse into the first target: stageSfi (six words per query, four per keypoint)"] = 6 * 4 * len(cur.slots) + 4 * 4 * len(targets[0].keys)
    out["Fuse, at most (every point a query of the second round): stageSfi"] = 6 * 4 * len(points) + 4 * 4 * max(len(k.keys) for k in [cur] + targets)
    out["projection search, 43 queries: stageSfi (64 + 256 list words, a count and an overflow word per query)"] = 43 * (64 * 4 + 2 + 4 + 256 * 4)
    return out
