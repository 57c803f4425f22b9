"""K4-6's front (its 96-byte argument block, compile-time blur taps, the one constant table, the window fetch ahead of the
table loads) against the CPU oracle, byte for byte: keypoints, descriptors and counts.

Small odd-sized frames (w & ~3 != w) put a good share of the keypoints 19-20 px from a border, i.e. on the reflect-101 path,
the rest on the LDS-DMA path; both blur tie modes; an output capacity below a frame's count (the idx < cap guard); level-range
launches (slotBeg / slotEnd / writeTotal through the block); and a nearly flat frame whose levels keep fewer keypoints than
their capacity (marked records)."""
import ctypes as C

import numpy as np
import pytest

from pilotguru_amd.synth import synth_scene

pytestmark = pytest.mark.gpu

SIZES = [(200, 160), (131, 97)]
NF, NL, B = 300, 3, 3


def _frames(w, h):
    return np.stack([synth_scene(70 + f, w, h) for f in range(B)])


def _flat_frames(w, h):
    """Constant grey with a few bright squares: a handful of corners per frame, far fewer than any level's capacity."""
    out = np.full((B, h, w), 90, np.uint8)
    for f in range(B):
        for k in range(3 + f):
            x, y = 30 + 37 * k + 5 * f, 28 + 23 * k + 3 * f
            out[f, y:y + 9, x:x + 11] = 200
    return out


_want = {}


def _oracle(oracle, key, frames, tie):
    """The oracle's (keypoints, descriptors) per frame, computed once per (scene, tie mode) and shared."""
    k = (key, tie)
    if k not in _want:
        ora = oracle.OrbOracle(NF, 1.2, NL, 20, 7, blur_tie_mode=tie)
        _want[k] = [ora.extract(f) for f in frames]
    return _want[k]


def _ext(w, h, tie):
    import pilotguru_amd as pg
    return pg.ORBextractor(NF, 1.2, NL, 20, 7, max_width=w, max_height=h, max_batch=B, blur_tie_mode=tie)


def _check_device(ext, frames, want):
    import torch
    kps, desc, n = ext.extract_batch_device(torch.from_numpy(frames).cuda())
    ext.check_async()
    torch.cuda.synchronize()
    nh = n.cpu().numpy()
    for f in range(len(frames)):
        okp, odesc = want[f]
        assert nh[f] == len(okp)
        assert kps[f, :nh[f]].cpu().numpy().tobytes() == okp.tobytes()
        assert np.array_equal(desc[f, :nh[f]].cpu().numpy(), odesc)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("tie", [0, 1])
def test_front_bit_exact_both_paths(oracle, w, h, tie):
    frames = _frames(w, h)
    want = _oracle(oracle, (w, h), frames, tie)
    # the scene exercises both staging paths: keypoints whose 48-byte window rows leave the level (reflect-101) and inside ones
    okp = want[0][0]
    lvl0 = okp[okp["octave"] == 0]
    x0, y0 = lvl0["x"].astype(int) - 21, lvl0["y"].astype(int) - 21
    inside = (x0 >= 0) & (y0 >= 0) & (x0 + 48 <= w) & (lvl0["y"].astype(int) + 21 < h)
    assert inside.any() and (~inside).any()
    _check_device(_ext(w, h, tie), frames, want)


@pytest.mark.parametrize("w,h", SIZES)
def test_front_output_capacity_below_count(oracle, w, h):
    """cap_per_frame < a frame's count: the count is reported whole, the first cap outputs are the reference's, nothing past them is written."""
    import torch
    frames = _frames(w, h)
    want = _oracle(oracle, (w, h), frames, 0)
    cap = min(len(k) for k, _ in want) // 2
    assert cap >= 8
    ext = _ext(w, h, 0)
    guard = 4
    kps = torch.full((B * cap + guard, 7), -7.0, dtype=torch.float32, device="cuda")
    desc = torch.full((B * cap + guard, 32), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.zeros((B,), dtype=torch.int32, device="cuda")
    fr = torch.from_numpy(frames).cuda()
    s = torch.cuda.current_stream().cuda_stream
    ext._check(ext._L.pgorb_extract_batch_device(
        ext._h, C.c_void_p(fr.data_ptr()), B, w, h, fr.stride(1), fr.stride(0), C.c_void_p(kps.data_ptr()),
        C.c_void_p(desc.data_ptr()), cap, C.c_void_p(n.data_ptr()), C.c_void_p(s)))
    torch.cuda.synchronize()
    nh, kh, dh = n.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
    for f in range(B):
        okp, odesc = want[f]
        assert nh[f] == len(okp) and len(okp) > cap
        assert kh[f * cap:(f + 1) * cap].tobytes() == okp[:cap].tobytes()
        assert np.array_equal(dh[f * cap:(f + 1) * cap], odesc[:cap])
    assert np.all(kh[B * cap:] == -7.0) and np.all(dh[B * cap:] == 0xA5)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mask", [0b10, 0b110])
def test_front_level_range_launches(oracle, w, h, mask):
    """pipeline_levels: K4-6 launched per range of levels ([0], [1, 2] and one level each), then the single launch again."""
    frames = _frames(w, h)
    want = _oracle(oracle, (w, h), frames, 0)
    ext = _ext(w, h, 0)
    for m in (mask, 0):
        ext.set_option("pipeline_levels", m)
        _check_device(ext, frames, want)


@pytest.mark.parametrize("tie", [0, 1])
def test_front_marked_records(oracle, tie):
    """A nearly flat batch: every level keeps fewer keypoints than its capacity, so most slots hold marked records."""
    w, h = SIZES[0]
    frames = _flat_frames(w, h)
    want = _oracle(oracle, "flat", frames, tie)
    counts = [len(k) for k, _ in want]
    assert all(0 < c < NF // 4 for c in counts), counts
    ext = _ext(w, h, tie)
    _check_device(ext, frames, want)
    ext.set_option("pipeline_levels", 0b110)
    _check_device(ext, frames, want)
