"""bench.py --dump-outputs on host tensors shaped like the timed path's buffers: the caller's layout, by-value
keypoint fields, nothing past n[f], and a seeded frame sample that keeps the dump under its byte limit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pilotguru_amd.orb import KEYPOINT_DTYPE  # noqa: E402


def _buffers(B=6, cap=50):
    r = np.random.default_rng(1)
    rec = np.zeros((B, cap), KEYPOINT_DTYPE)
    for f in KEYPOINT_DTYPE.names:
        rec[f] = r.integers(-5, 1000, (B, cap))
    kps = torch.from_numpy(rec.view(np.float32).reshape(B, cap, 7).copy())
    desc = torch.from_numpy(r.integers(0, 256, (B, cap, 32)).astype(np.uint8))
    n = torch.from_numpy(np.array([cap, 3, 0, 20, cap - 1, 10][:B], np.int32))
    mout = (torch.from_numpy(r.integers(-1, cap, (B - 1, cap)).astype(np.int32)),
            torch.from_numpy(r.integers(-1, 256, (B - 1, cap)).astype(np.int16)),
            torch.from_numpy(r.integers(-1, 256, (B - 1, cap)).astype(np.int16)))
    return rec, kps, desc, n, mout


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_whole_batch(tmp_path):
    rec, kps, desc, n, mout = _buffers()
    info = bench.dump_outputs(str(tmp_path), kps, desc, n, mout)
    o = _load(str(tmp_path))
    assert info["frames"] == info["of_frames"] == 6 and sorted(o) == info["arrays"]
    assert all(a.dtype in (np.float32, np.float64) for a in o.values())
    assert info["bytes"] == sum(a.nbytes for a in o.values())
    nh = n.numpy()
    assert np.array_equal(o["frames"], np.arange(6)) and np.array_equal(o["n_keypoints"], nh)
    for f in range(6):
        k = nh[f]
        for j, name in enumerate(KEYPOINT_DTYPE.names):
            assert np.array_equal(o["keypoints"][f, :k, j], rec[name][f, :k].astype(np.float64))
        assert np.array_equal(o["descriptors"][f, :k], desc[f, :k].numpy())
        assert not o["keypoints"][f, k:].any() and not o["descriptors"][f, k:].any()
    assert np.array_equal(o["match_query_frames"], np.arange(1, 6))
    for p in range(5):
        k = nh[p + 1]
        for name, t in zip(("match_best_idx", "match_best_dist", "match_second_dist"), mout):
            assert np.array_equal(o[name][p, :k], t[p, :k].numpy()) and not o[name][p, k:].any()


def test_dump_outputs_samples_frames_under_the_limit(tmp_path, monkeypatch):
    rec, kps, desc, n, mout = _buffers()
    cap = kps.shape[1]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * (cap * (7 * 8 + 32 * 4) + 16 + cap * 16 + 8))
    dirs = [os.path.join(str(tmp_path), s) for s in ("a", "b")]
    for d in dirs:
        info = bench.dump_outputs(d, kps, desc, n, mout)
        assert info["frames"] == 3 and info["bytes"] <= bench.DUMP_LIMIT_BYTES
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)     # the same sample every run
    fr = a["frames"].astype(int)
    assert len(set(fr)) == 3 and np.all(np.diff(fr) > 0)
    assert np.array_equal(a["n_keypoints"], n.numpy()[fr])
    assert np.array_equal(a["match_query_frames"], fr[fr >= 1])
    q = fr[fr >= 1]
    k = n.numpy()[q[0]]
    assert np.array_equal(a["match_best_idx"][0, :k], mout[0][q[0] - 1, :k].numpy())
