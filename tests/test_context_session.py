"""One long-lived context, as the library is used: calls of every family on ONE pgorb_ctx, which share its arenas
(stageA, the page-locked buffer, stageSfi, stageOut, xdesc, outBlk and the plan arenas, vocab), the captured extract graph and the
scratch ordering across caller streams.  tests/session_cases.py holds the schedules; every step is compared, exactly, with its
family's CPU reference, after a synchronisation and pgorb_check_async of its own, and every step that is meant to reallocate an
arena -- or to leave it alone -- is shown to have done so through pgorb_debug_arena."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import session_cases as SC  # noqa: E402



def limit(seconds):
    """The test's own time limit: SIGALRM raises inside it (a test stuck in a HIP call is left to the caller's limit)."""
    import functools
    import signal

    def wrap(fn):
        @functools.wraps(fn)
        def run(*a, **k):
            def stop(*_):
                raise TimeoutError("%s ran longer than %d s" % (fn.__name__, seconds))
            old = signal.signal(signal.SIGALRM, stop)
            signal.alarm(seconds)
            try:
                return fn(*a, **k)
            finally:
                signal.alarm(0)
                signal.signal(signal.SIGALRM, old)
        return run
    return wrap

ALL = [(name, make()) for name, make in SC.SCHEDULES.items()]


# ---------------------------------------------------------------- CPU: the schedules themselves
def test_symbols_and_null_context():
    import ctypes as C
    from pilotguru_amd import _lib
    L = _lib.lib()
    for name in ("pgorb_debug_arena", "pgorb_debug_host_graph"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    p, n, a, b = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_int32()
    assert L.pgorb_debug_arena(None, 0, C.byref(p), C.byref(n)) == -1 and L.pgorb_debug_host_graph(None, C.byref(a), C.byref(b)) == -1


@pytest.mark.parametrize("name,steps", ALL, ids=[n for n, _ in ALL])
def test_schedule_is_well_formed(name, steps):
    assert len(steps) >= 3 and len(set(s.name for s in steps)) == len(steps)
    for s in steps:
        assert s.form in SC.FORMS[s.family], s
        assert s.stream in (None, "A", "B") and s.ctx in (0, 1)
        assert set(s.edges) <= set(SC.EDGES), s
        assert set(s.grow) | set(s.still) <= set(SC.ARENAS) and not set(s.grow) & set(s.still), s
        assert s.stream is None or s.form == "device", "only the *_batch_device forms take a stream: %r" % (s,)


def test_every_edge_is_declared_and_none_unused():
    seen = collections.Counter(e for _, steps in ALL for s in steps for e in s.edges)
    assert not [e for e in SC.EDGES if not seen[e]], "undeclared"
    assert not [e for e in seen if e not in SC.EDGES], "unknown"
    grown = {a for n in ("a", "a_plan") for s in dict(ALL)[n] for a in s.grow}
    stilled = {a for n in ("a", "a_plan") for s in dict(ALL)[n] for a in s.still}
    assert grown == set(SC.ARENAS) and stilled == set(SC.ARENAS), "every arena is grown, and left alone, by some step of (a)"


def test_every_replay_condition_has_a_step():
    """Each condition of HostGraph's replay (extract.hip) is answered for by a step of (b) that declares its edge and states which
    way its extract must run."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pilotguru_amd", "csrc", "extract.hip")).read()
    line = [ln for ln in src.splitlines() if "const bool replay =" in ln][0]
    for cond, edge in SC.REPLAY_CONDITIONS.items():
        assert cond in line, cond
        assert [s for s in dict(ALL)["b"] if edge in s.edges], edge
    assert line.count("==") == len(SC.REPLAY_CONDITIONS), "a replay condition without a step of (b): %s" % line


@pytest.mark.parametrize("name,steps", ALL, ids=[n for n, _ in ALL])
def test_no_step_is_vacuous(oracle, name, steps):
    prev = {}
    for s in steps:
        s = SC.plain(s)
        if s.family in SC.CHECKED:
            assert SC.nontrivial(s.family, s.case, SC.reference(s.family, s.case, oracle)), s
        last = prev.get((s.ctx, s.family))
        assert last is None or last[0] != s.case or last[1] != steps.index(SC_orig(steps, s)) - 1, \
            "two consecutive steps of one family with the same case: %r" % (s,)
        prev[(s.ctx, s.family)] = (s.case, steps.index(SC_orig(steps, s)))


def SC_orig(steps, plain):
    return next(s for s in steps if s.name == plain.name)


def test_large_means_past_the_rounding_and_the_head_room():
    z = SC.sizes()
    grow = lambda small, large: large > small + (small >> 2) + 4096
    assert grow(z["best2 300x400: xdesc (2 KiB per 16 train descriptors and pair)"], z["match_batch 4x2000x3: xdesc"])
    assert grow(z["best2 300x400: stageA = pinned request"], z["refresh of the neighbourhood: stageA = pinned request"])
    assert grow(z["SearchByBoW, 22 keypoints: stageSfi (a byte per keypoint)"], z["Fuse into the first target: stageSfi (six words per query, four per keypoint)"])
    assert z["projection search, 43 queries: stageSfi (64 + 256 list words, a count and an overflow word per query)"] > \
        z["Fuse, at most (every point a query of the second round): stageSfi"] + 4096            # (ensure() keeps no head-room)
    assert z["best2 30000x500: download"] > 60 * 3000          # more than an extract's download at 320 x 240 (60 B per keypoint)


# ---------------------------------------------------------------- GPU
def _contexts(n=1, schedule=None):
    import pilotguru_amd as pg
    return [SC.make_context(pg, **SC.CONTEXT.get(schedule, {})) for _ in range(n)]


def _close(ctx):
    for c in ctx:
        c.close()


@pytest.mark.gpu
@limit(120)
@pytest.mark.parametrize("schedule", ["a", "a_plan"])
def test_gpu_grow_shrink_regrow_of_every_arena(oracle, schedule):
    ctx = _contexts(1, schedule)
    ses = SC.Session(ctx, oracle)
    try:
        ses.run(dict(ALL)[schedule])
    finally:
        print(ses.log)
        _close(ctx)


@pytest.mark.gpu
@limit(60)
def test_gpu_captured_graph_against_what_invalidates_it(oracle):
    ctx = _contexts(1, "b")
    ses = SC.Session(ctx, oracle)
    same_address = None
    try:
        for st in dict(ALL)["b"]:
            before, after = ses.step(SC.plain(st))
            if st.name == "matcher_download":
                moved = before["pinned"], after["pinned"]
            if st.family != "extract":
                continue
            last, _ = ctx[0].debug_host_graph()
            want = st.case[1]
            if st.name == "after_pinned_moved":
                # the buffer was freed and allocated again, larger: a replay is right only if it came back at the address the
                # graph holds (the allocator decides; recorded, not forced)
                same_address = moved[0][0] == moved[1][0]
                assert last in ((2,) if same_address else (0, 1)), "%s: ran as %d, buffer at the same address: %s" % (ses.where(st), last, same_address)
            else:
                assert last == want, "%s: ran as %d, expected %d (0 direct, 1 captured, 2 replayed)" % (ses.where(st), last, want)
    finally:
        print("page-locked buffer came back at the same address:", same_address, ses.log)
        _close(ctx)


def _queued_schedule(ses, steps, streams):
    """Queue every step without a host synchronisation in between, synchronise once, then collect and compare in order."""
    import torch
    pending = []
    with SC.Queued.patched():
        try:
            for st in steps:
                ext = ses.ctx[st.ctx]
                q = SC.Queued(lambda st=st, ext=ext: SC.run(st, ext), streams[st.stream], SC.PARK_AT.get(st.family, 1))
                pending.append((st, q.start()))
            SC.Queued._real()
        finally:
            got = []
            for st, q in pending:
                got.append((st, q.finish()))
    for st, g in got:
        ses.sync(st, ses.ctx[st.ctx])
        ses.check(st, g)
        ses.index, ses.prev = ses.index + 1, st.name


@pytest.mark.gpu
@limit(60)
@pytest.mark.parametrize("null_stream", [False, True])
def test_gpu_two_caller_streams_without_host_synchronisation(oracle, null_stream):
    import torch
    ctx = _contexts()
    ses = SC.Session(ctx, oracle)
    try:
        streams = {"A": torch.cuda.Stream(), "B": None if null_stream else torch.cuda.Stream(), None: None}
        steps = dict(ALL)["c_null" if null_stream else "c"]
        _queued_schedule(ses, steps, streams)
        _queued_schedule(ses, steps[::-1], streams)              # and B before A, on arenas that no longer grow
    finally:
        _close(ctx)


@pytest.mark.gpu
@limit(90)
def test_gpu_streams_alive_while_the_arenas_grow(oracle):
    """A FrameStream and a DeviceFrameStream on the context: submit, steps that regrow xdesc and stageA (match_mode 0 set after the
    streams exist), wait, compare with the oracle, submit again."""
    import numpy as np
    import torch
    import pilotguru_amd as pg
    from pilotguru_amd.synth import synth_ride
    w, h = 640, 480
    ride = synth_ride(9, w, h, 8)
    ctx = _contexts()
    ses = SC.Session(ctx, oracle)
    fs, ds = pg.FrameStream(ctx[0], w, h, 4, 2), pg.DeviceFrameStream(ctx[0], w, h, 4, 2, 2)
    ora = oracle.OrbOracle(SC.NFEATURES, 1.2, 8, 20, 7)
    want = [ora.extract(f) for f in ride]
    frames = torch.from_numpy(ride).cuda()
    steps = dict(ALL)["d"]
    try:
        for blk in range(2):
            # (the two streams share the context's one working set: one batch in flight at a time)
            between = steps if blk == 0 else [s._replace(grow=()) for s in steps[1:]]
            fs.input(blk)[:4] = ride[4 * blk:4 * blk + 4]
            fs.submit(blk, 4)
            for st in between[:2]:
                ses.step(st)
            rn, rk, rd, rbi, rb1, rb2 = fs.wait(blk)
            ds.submit(blk, frames[4 * blk:4 * blk + 4])
            for st in between[2:]:
                ses.step(st)
            dn, dk, dd, dbi, db1, db2 = ds.wait(blk)
            torch.cuda.synchronize()
            for f in range(4):
                okp, odesc = want[4 * blk + f]
                n = len(okp)
                where = "block %d frame %d after '%s'" % (blk, f, ses.prev)
                assert int(rn[f]) == n and np.array_equal(rd[f, :n], odesc) and rk[f, :n].tobytes() == okp.tobytes(), "FrameStream " + where
                assert int(dn[f]) == n and np.array_equal(dd[f, :n].cpu().numpy(), odesc), "DeviceFrameStream " + where
                if blk or f:
                    obi, ob1, ob2 = oracle.hamming_best2(odesc, want[4 * blk + f - 1][1])
                    assert np.array_equal(rbi[f, :n], obi) and np.array_equal(rb1[f, :n], ob1) and np.array_equal(rb2[f, :n], ob2), "FrameStream match " + where
                    assert np.array_equal(dbi[f, :n].cpu().numpy(), obi) and np.array_equal(db1[f, :n].cpu().numpy().view(np.uint16), ob1), \
                        "DeviceFrameStream match " + where
            del rn, rk, rd, rbi, rb1, rb2, dn, dk, dd, dbi, db1, db2
    finally:
        fs.close(); ds.close()
        _close(ctx)


@pytest.mark.gpu
@limit(90)
def test_gpu_two_contexts_alternating(oracle):
    ctx = _contexts(2)
    ses = SC.Session(ctx, oracle)
    try:
        ses.run(dict(ALL)["e"])
        assert ctx[0].get_option("match_mode") == 0 and ctx[1].get_option("match_mode") == -1
    finally:
        _close(ctx)


@pytest.mark.gpu
@limit(60)
def test_gpu_destroy_a_context_while_another_has_queued_work(oracle):
    import torch
    ctx = _contexts(2)
    ses = SC.Session(ctx, oracle)
    first, other, last = dict(ALL)["f"]
    s = torch.cuda.Stream()
    try:
        with SC.Queued.patched():
            qa = SC.Queued(lambda: SC.run(first, ctx[0]), s).start()              # queued on context 0's stream, not waited for
            try:
                got = SC.run(other, ctx[1])
                ctx[1].close()                                                    # pgorb_destroy while context 0 has work in flight
                qb = SC.Queued(lambda: SC.run(last, ctx[0]), s).start()
                SC.Queued._real()
            finally:
                ga = qa.finish()
            gb = qb.finish()
        ses.check(other, got)
        for st, g in ((first, ga), (last, gb)):
            ses.sync(st, ctx[0])
            ses.check(st, g)
    finally:
        _close(ctx)
