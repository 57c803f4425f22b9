"""Constructed edge cases of the extractor (tests/extractor_cases.py), checked against an independent plain reference
(tests/extractor_reference.py) as well as the oracle (oracle/orb_oracle.c).

On the CPU each family must reach its target edges (a hit count > 0), the reference must equal the oracle byte for byte, and
every wrong reading of a rule (extractor_reference.MUTANTS) must change the output of at least one case -- except the one
mutant shown here to be equivalent.  On the GPU every case runs through pgorb_extract (graph replay included), the fused K1+K2
launch, other K2 tile shapes and both K3 forms, and through pgorb_extract_batch_device on caller buffers with poisoned
padding, level 0 aliasing them."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extractor_reference as R  # noqa: E402
from extractor_cases import FAMILIES, TARGETS, all_cases, fused_variant, run_oracle, run_reference, same  # noqa: E402

# a wrong reading no output can tell from the reference: a column the "-3" reading keeps has iniX >= maxBorderX - 6, so its
# window (clipped at maxBorderX) is at most 6 columns wide, and cv::FAST tests nothing in a window narrower than 7.  The row rule's
# asymmetry (:794, iniY >= maxBorderY - 3) is unobservable for the same reason: a row it keeps in [maxBorderY - 6, maxBorderY - 3)
# has a window of at most 6 rows.  The hits cell_skip_x / cell_row_kept_in_x_skip_zone only show that the frames reach that zone.
EQUIVALENT = {"skip_x=3"}


@pytest.fixture(scope="module")
def solved(oracle):
    """Every case with the oracle's output and level images, and the reference's output with its hit counts."""
    out = []
    for case in all_cases(0):
        kps, desc, levels = run_oracle(case, oracle)
        hits = collections.Counter()
        want = run_reference(case, levels, hits=hits)
        out.append((case, (kps, desc), levels, want, hits))
    return out


# ---------------------------------------------------------------- CPU: reference == oracle, hit counts, mutants
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_reference_equals_oracle_on_constructed_family(solved, family):
    hits = collections.Counter()
    rows = [r for r in solved if r[0]["family"] == family]
    assert rows
    for case, got, _, want, h in rows:
        hits.update(h)
        assert same(want, got), "%s: reference (%d keypoints) != oracle (%d)" % (case["name"], len(want[0]), len(got[0]))
        assert len(want[0]) > 0, case["name"]
    missed = [t for t in TARGETS[family] if hits[t] == 0]
    assert not missed, "family %s never reached %s (hits %s)" % (family, missed, dict(hits))


def test_every_rule_mutant_is_caught(solved):
    missed = []
    for name, rules in R.MUTANTS.items():
        caught = [case["name"] for case, _, levels, want, _ in solved if not same(run_reference(case, levels, rules), want)]
        if name in EQUIVALENT:
            assert not caught, "mutant %s was declared equivalent but changes %s" % (name, caught)
        elif not caught:
            missed.append(name)
    assert not missed, "mutants no constructed case catches: %s" % missed


def test_skip_x_mutant_is_equivalent_where_it_applies(solved):
    """The windows the skip_x=3 reading adds exist in the constructed frames, and every one is under 7 columns wide."""
    added = 0
    for case, _, levels, _, _ in solved:
        for img in levels:
            h, w = img.shape
            ref = {(c[0], c[1]) for c in R.level_cells(w, h)[0]}
            for c in R.level_cells(w, h, R.MUTANTS["skip_x=3"])[0]:
                if (c[0], c[1]) not in ref:
                    added += 1
                    assert c[4] - c[2] < 7, (case["name"], c)
    assert added > 0


def test_reference_tables_and_primitives_by_hand(oracle):
    """Constructor tables and the contract primitives at their branch points, stated from the upstream text."""
    o = oracle.OrbOracle(2000, 1.2, 8, 20, 7)
    assert R.features_per_level(2000, 1.2, 8) == o.features_per_level.tolist()
    assert R.umax_table() == o.umax.tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert R.umax_table(R.MUTANTS["umax=floor"])[1] == 14
    assert np.array_equal(R.scale_factors(1.2, 8), o.scale_factors)
    assert np.array_equal(R.scale_factors(2.0, 3), oracle.OrbOracle(500, 2.0, 3, 20, 7).scale_factors)
    for y, x in ((0, 0), (0, 5), (0, -5), (5, 0), (-5, 0), (7, 7), (-7, 7), (7, -7), (-7, -7), (3, -2), (1000, 1)):
        assert R.fast_atan2(y, x) == np.float32(oracle.fast_atan2(y, x)), (y, x)
    assert R.fast_atan2(30, 30) != R.fast_atan2(30, 30, R.MUTANTS["atan_branch=gt"])
    for a in np.linspace(0, 2 * np.pi, 997).astype(np.float32):
        s, c = oracle.sincos_f(a)
        assert R.contract_sincos(a) == (np.float32(s), np.float32(c))
    for tie in (0, 1):
        rng = np.random.RandomState(tie)
        img = rng.randint(0, 256, (23, 30)).astype(np.uint8)
        assert np.array_equal(R.gaussian_blur7(img, tie)[0], oracle.gaussian_blur7(img, tie))


def test_reference_equals_oracle_on_synthetic_scenes(oracle):
    """Natural content too: synthetic scenes through the whole extractor, both blur tie modes, two scale factors."""
    from pilotguru_amd.synth import synth_scene
    for (seed, w, h, nf, sf, nl, tie) in ((1, 320, 240, 500, 1.2, 3, 0), (2, 200, 150, 300, 2.0, 2, 0), (3, 257, 181, 400, 1.2, 3, 1)):
        o = oracle.OrbOracle(nf, sf, nl, 20, 7, blur_tie_mode=tie)
        got = o.extract(synth_scene(seed, w, h))
        want = R.extract([o.level_image(l) for l in range(nl)], nf, sf, nl, 20, 7, tie)
        assert same(want, got) and len(want[0]) > 100


# ---------------------------------------------------------------- GPU
def _key(case):
    h, w = case["img"].shape
    return (case["nfeatures"], case["scale"], case["nlevels"], case["ini"], case["min"], case["tie"], w, h)


def _extractor(case, batch=1, **options):
    import pilotguru_amd as pg
    nf, sf, nl, ini, mn, tie, w, h = _key(case)
    ext = pg.ORBextractor(nf, sf, nl, ini, mn, max_width=w, max_height=h, max_batch=batch, blur_tie_mode=tie)
    for k, v in options.items():
        ext.set_option(k, v)
        assert ext.get_option(k) == v, k
    return ext


def _gpu_cases(oracle):
    """(case, reference output, fused variant, its reference output) for every constructed case."""
    out = []
    for case in all_cases(0):
        fcase = fused_variant(case)
        res = []
        for c in (case, fcase):
            _, _, levels = run_oracle(c, oracle)
            res += [c, run_reference(c, levels)]
        out.append(tuple(res))
    return out


@pytest.fixture(scope="module")
def gpu_cases(oracle):
    return _gpu_cases(oracle)


def _check(case, got, want, label):
    assert same(want, got), "%s (%s): kernel %d keypoints, reference %d" % (case["name"], label, len(got[0]), len(want[0]))


def _fused_taken(ext, case):
    """The last batch ran level 0 (at least) through the fused resize + detect launch."""
    assert ext.get_option("fused_levels") == 1
    assert ext.get_option("fused_launches") >= 1, "%s: the fused launch was not taken" % case["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("options", [{}, {"fused_levels": 1},
                                     {"fused_levels": 0, "fast_tile_pitch": 64, "fast_waves_per_block": 4, "fast_cells_per_wave": 3},
                                     {"quadtree_split": 0}, {"quadtree_split": 1}],
                         ids=["default", "fused", "k2_shape", "qt_one_launch", "qt_split"])
def test_kernels_equal_reference_on_constructed_cases(gpu_cases, options):
    """pgorb_extract three times per case (the second call captures a graph, the third replays it).  With fused_levels = 1 every
    case runs as its fused variant (>= 2 levels), and the fused launch must have been taken."""
    fused = options.get("fused_levels") == 1
    for row in gpu_cases:
        case, want = row[2:] if fused else row[:2]
        ext = _extractor(case, **options)
        try:
            for k in range(3):
                _check(case, ext(case["img"]), want, "%s call %d" % (options, k))
                if fused and k == 0:
                    _fused_taken(ext, case)
        finally:
            ext.close()


@pytest.mark.gpu
def test_kernels_equal_reference_with_blur_tie_mode_1(oracle, gpu_cases):
    """Family f again with blur_tie_mode = 1 (the cases with tie 0, re-run under the other mode against the reference)."""
    for case, _, _, _ in gpu_cases:
        if case["family"] != "f" or case["tie"] != 0:
            continue
        c = dict(case, tie=1)
        _, _, levels = run_oracle(c, oracle)
        want = run_reference(c, levels)
        ext = _extractor(c)
        try:
            _check(c, ext(c["img"]), want, "tie 1")
        finally:
            ext.close()


def _groups(pairs):
    g = collections.OrderedDict()
    for case, want in pairs:
        g.setdefault(_key(case), []).append((case, want))
    return list(g.values())


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("pitch_mod", [0, 4])
def test_batch_device_on_aliased_poisoned_buffers(gpu_cases, fused, pitch_mod):
    """pgorb_extract_batch_device on the cases of one geometry packed as one batch: level 0 aliases the caller's buffer, whose
    row pitch is = pitch_mod (mod 16) and whose bytes between w and the pitch, and between frames, hold 0x00, 0xFF or noise; the
    buffer ends with the w bytes of the last frame's last row.  Frames of a group repeat so every group is a batch of at least 2.
    fused = 1 runs the fused variants, and the fused launch must have been taken on the caller's rows."""
    import torch
    rng = np.random.RandomState(16 * fused + pitch_mod)
    for group in _groups([row[2:] if fused else row[:2] for row in gpu_cases]):
        case0 = group[0][0]
        h, w = case0["img"].shape
        items = group * (2 if len(group) == 1 else 1)
        B = len(items)
        pitch = ((w + 15) & ~15) + pitch_mod
        fstride = h * pitch + 64
        poison = rng.choice(["zero", "ff", "noise"])
        buf = {"zero": np.zeros, "ff": lambda n, dt: np.full(n, 255, dt)}.get(poison, lambda n, dt: rng.randint(0, 256, n).astype(dt))(
            (B - 1) * fstride + (h - 1) * pitch + w, np.uint8)
        for k, (case, _) in enumerate(items):
            for y in range(h):
                buf[k * fstride + y * pitch:k * fstride + y * pitch + w] = case["img"][y]
        dev = torch.from_numpy(buf).cuda()
        view = torch.as_strided(dev, (B, h, w), (fstride, pitch, 1))
        ext = _extractor(case0, batch=B, fused_levels=fused)
        try:
            kps, desc, n = ext.extract_batch_device(view)
            ext.check_async()
            torch.cuda.synchronize()
            if fused:
                _fused_taken(ext, case0)
            kps, desc, n = kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy()
            for k, (case, want) in enumerate(items):
                got = (kps[k, :n[k]].copy().view(R.KEYPOINT_DTYPE).reshape(-1), desc[k, :n[k]])
                _check(case, got, want, "batch fused %d pitch %d poison %s frame %d" % (fused, pitch, poison, k))
        finally:
            ext.close()
