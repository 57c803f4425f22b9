"""Constructed frames for the extractor's edge cases (tests/test_extractor_edges.py), in families a-h.  Every frame is built
from a flat grey canvas with isolated features whose FAST contrast, position and patch moments are chosen, so the rules of
ORBextractor.cc that decide which keypoints come out (thresholds, the per-cell retry, NMS, the cell grid, candidate order, the
quadtree, IC_Angle, the blur border and rBRIEF) are reached on purpose.  The full keypoint set is not predicted by hand:
features create side corners, and the reference, the oracle and the kernels must agree on those too.  TARGETS names the
`hits` keys (extractor_reference) each family must reach.

A case is a dict: name, family, img (uint8 [h, w]), nfeatures, scale, nlevels, ini, min, tie (blur_tie_mode).  Every frame size
gives cells of 16 .. 32 x 16 .. 40 px, the geometry the fused resize + detect launch takes (fused.hip), so `fused_variant` of a case
runs its edge cases through that launch's detector."""
import numpy as np

import extractor_reference as R

BG = 128
INI, MIN = 20, 7


def canvas(w, h, bg=BG):
    return np.full((h, w), bg, np.uint8)


def dot(img, x, y, c, bg=None):
    """One pixel of contrast c against the canvas: a FAST corner of arc contrast |c| (its whole ring is background)."""
    base = int(img[y, x]) if bg is None else bg
    img[y, x] = np.uint8(min(255, max(0, base + c)))


def case(family, name, img, nfeatures=200, scale=1.2, nlevels=1, ini=INI, mn=MIN, tie=0):
    return {"family": family, "name": name, "img": img, "nfeatures": nfeatures, "scale": scale, "nlevels": nlevels,
            "ini": ini, "min": mn, "tie": tie}


def cell_geometry(w, h):
    """(cells, borders) of a w x h level as ComputeKeyPointsOctTree walks them."""
    return R.level_cells(w, h)


def cell_interior(w, h, i, j):
    """Absolute (x_first, x_last, y_first, y_last) of the pixels cell (i, j)'s window tests (its 3-px ring excluded)."""
    cells, _ = R.level_cells(w, h)
    for (ci, cj, x0, y0, x1, y1, _, _) in cells:
        if (ci, cj) == (i, j):
            return x0 + 3, x1 - 4, y0 + 3, y1 - 4
    raise KeyError((i, j))


def arc(img, x, y, start, length, c):
    """Centre (x, y) left at the canvas value, `length` contiguous ring pixels from ring index `start` (wrapping 15 -> 0) set
    c below it: an arc of `length` darker pixels."""
    for k in range(length):
        dx, dy = R.RING[(start + k) % 16]
        img[y + dy, x + dx] = np.uint8(max(0, int(img[y, x]) - c))


# ---------------------------------------------------------------- a. thresholds and the retry
def family_a(rng):
    w, h = 212, 150                                    # 6 x 3 cells of 30 x 40
    out = []
    img = canvas(w, h)
    x0, x1, y0, y1 = cell_interior(w, h, 0, 0)
    dot(img, x0 + 10, y0 + 10, INI)                    # arc contrast == iniTh: not a corner at iniTh, the cell retries
    x0, x1, y0, y1 = cell_interior(w, h, 0, 1)
    dot(img, x0 + 8, y0 + 8, INI + 1)                  # iniTh + 1: found at iniTh ...
    dot(img, x0 + 20, y0 + 20, INI)                    # ... so this one (== iniTh) must stay out
    x0, x1, y0, y1 = cell_interior(w, h, 0, 2)
    dot(img, x0 + 12, y0 + 6, MIN)                     # == minTh: never a corner
    x0, x1, y0, y1 = cell_interior(w, h, 0, 3)
    dot(img, x0 + 5, y0 + 14, MIN + 1)                 # minTh + 1: found by the retry
    x0, x1, y0, y1 = cell_interior(w, h, 0, 4)
    dot(img, x0 + 9, y0 + 9, -(INI + 1))               # dark
    dot(img, x0 + 20, y0 + 25, -INI)
    x0, x1, y0, y1 = cell_interior(w, h, 1, 0)
    img[y0 + 8:y0 + 14, x0 + 8:x0 + 14] = BG + 40      # a square: its corners are equal-score plateaus -> NMS empties the cell
    x0, x1, y0, y1 = cell_interior(w, h, 1, 1)
    arc(img, x0 + 8, y0 + 8, 12, 9, 30)                # arc of exactly 9, wrapping 15 -> 0
    arc(img, x0 + 22, y0 + 22, 13, 8, 30)              # arc of 8: the centre is no corner
    x0, x1, y0, y1 = cell_interior(w, h, 1, 2)
    dot(img, x0 + 15, y0 + 15, 12)                     # a minTh-only cell ...
    x0, x1, y0, y1 = cell_interior(w, h, 1, 3)
    dot(img, x0 + 15, y0 + 15, 45)                     # ... next to an iniTh cell
    x0, x1, y0, y1 = cell_interior(w, h, 2, 1)
    arc(img, x0 + 10, y0 + 10, 0, 9, INI)              # arc of 9 at exactly iniTh, then at minTh + 1
    arc(img, x0 + 24, y0 + 20, 5, 9, MIN + 1)
    x0, x1, y0, y1 = cell_interior(w, h, 2, 3)
    img[y0 + 5:y0 + 9, x0 + 5:x0 + 9] = BG + MIN + 1   # a plateau at minTh + 1 only: the retry finds nothing either
    out.append(case("a", "thresholds_and_retry", img))
    # the same frame with the thresholds moved: iniTh 12 == the minTh-only dot, minTh 8 == the minTh + 1 dot
    out.append(case("a", "thresholds_moved", img.copy(), ini=12, mn=8))
    # a frame whose every cell retries (no corner reaches iniTh anywhere)
    img = canvas(w, h)
    for k in range(12):
        dot(img, int(rng.randint(22, w - 22)), int(rng.randint(22, h - 22)), int(rng.choice([MIN, MIN + 1, INI - 1, INI])))
    out.append(case("a", "all_cells_retry", img))
    return out


# ---------------------------------------------------------------- b. NMS
def family_b(rng):
    w, h = 212, 150
    out = []
    img = canvas(w, h)
    x0, x1, y0, y1 = cell_interior(w, h, 0, 0)
    dot(img, x0 + 6, y0 + 6, 30)
    dot(img, x0 + 7, y0 + 6, 30)                       # orthogonal neighbours, equal scores: both go
    dot(img, x0 + 6, y0 + 20, 30)
    dot(img, x0 + 7, y0 + 21, 30)                      # diagonal neighbours, equal scores
    dot(img, x0 + 20, y0 + 20, 30)
    dot(img, x0 + 21, y0 + 20, 31)                     # unequal: the stronger stays
    # a stronger corner just across an interior boundary: both are kept (the ring scores 0 inside a window)
    _, xl, _, _ = cell_interior(w, h, 0, 1)
    dot(img, xl, y0 + 12, 25)                          # last tested column of cell (0, 1)
    dot(img, xl + 1, y0 + 12, 40)                      # first tested column of cell (0, 2)
    xa, _, _, yl = cell_interior(w, h, 0, 3)
    dot(img, xa + 10, yl, 25)                          # last tested row of cell row 0
    dot(img, xa + 10, yl + 1, 40)                      # first tested row of cell row 1
    dot(img, xa + 20, yl, 40)                          # and the other way round, diagonally
    dot(img, xa + 21, yl + 1, 25)
    # saturated score 254: 255 on 0
    x0, x1, y0, y1 = cell_interior(w, h, 2, 2)
    img[y0:y1 + 1, x0:x1 + 1] = 0
    img[y0 + 12, x0 + 12] = 255
    img[y0 + 20, x0 + 5] = 255
    img[y0 + 20, x0 + 6] = 255                         # a saturated equal pair
    out.append(case("b", "nms_ties_boundaries_saturation", img))
    img = canvas(w, h)                                 # random equal-score pairs and triples
    for k in range(25):
        x, y = int(rng.randint(22, w - 24)), int(rng.randint(22, h - 24))
        c = int(rng.choice([25, 30, -30]))
        for dx, dy in [(0, 0), (1, 0), (0, 1), (1, 1)][:int(rng.randint(1, 4))]:
            dot(img, x + dx, y + dy, c, BG)
    out.append(case("b", "nms_random_clusters", img))
    return out


# ---------------------------------------------------------------- c. cell geometry
def family_c(rng):
    out = []
    for (w, h) in ((903, 903), (870, 844), (843, 96), (93, 92), (125, 125), (320, 95)):
        img = canvas(w, h)
        (cells, (bx0, bx1, by0, by1)) = R.level_cells(w, h)
        for (x, y) in ((bx0 + 3, by0 + 3), (bx1 - 4, by0 + 3), (bx0 + 3, by1 - 4), (bx1 - 4, by1 - 4),
                       (bx0 + 3, (by0 + by1) // 2), (bx1 - 4, (by0 + by1) // 2 + 2), ((bx0 + bx1) // 2, by0 + 3),
                       ((bx0 + bx1) // 2 + 3, by1 - 4)):
            dot(img, x, y, int(rng.choice([25, -25, 12])))
        for (i, j, x0, y0, x1, y1, _, _) in cells[::max(1, len(cells) // 40)]:
            if x1 - x0 >= 7 and y1 - y0 >= 7:
                dot(img, int(rng.randint(x0 + 3, x1 - 3)), int(rng.randint(y0 + 3, y1 - 3)), int(rng.choice([22, 30, 10])))
        out.append(case("c", "geometry_%dx%d" % (w, h), img, nfeatures=300))
    return out


# ---------------------------------------------------------------- d. candidate order and the quadtree
def family_d(rng):
    out = []
    w, h = 212, 150
    # two equal responses in one final node: same cell row, the later column's corner higher up, so cell order and raster
    # order disagree on which one comes first (N = 1: the first division leaves both in one quadrant)
    img = canvas(w, h)
    xa, _, ya, _ = cell_interior(w, h, 0, 0)
    xb, _, yb, _ = cell_interior(w, h, 0, 1)
    dot(img, xa + 8, ya + 20, 30)
    dot(img, xb + 8, yb + 12, 30)
    out.append(case("d", "order_tie_one_node", img, nfeatures=1))
    img2 = img.copy()
    dot(img2, xb + 14, yb + 4, 30)                     # three of them
    out.append(case("d", "order_tie_three", img2, nfeatures=1))
    # N equal to the candidate count, one more and one less
    img = canvas(w, h)
    pts = set()
    while len(pts) < 14:
        pts.add((int(rng.randint(4, 40)) * 4 + 6, int(rng.randint(5, 30)) * 4 + 6))
    for (x, y) in pts:
        if 22 <= x < w - 22 and 22 <= y < h - 22:
            dot(img, x, y, int(rng.choice([25, 30, 35])))
    n = len(R.level_candidates(img, INI, MIN)[0])
    for d in (0, 1, -1):
        out.append(case("d", "quota_count%+d" % d, img.copy(), nfeatures=n + d))
    # more than one root node (wide frames), equal node sizes, many response ties
    for (w2, h2, nf) in ((320, 100, 20), (318, 96, 33), (320, 110, 7)):
        img = canvas(w2, h2)
        for k in range(60):
            dot(img, int(rng.randint(20, w2 - 20)), int(rng.randint(20, h2 - 20)), int(rng.choice([25, 30])))
        out.append(case("d", "roots_%dx%d_N%d" % (w2, h2, nf), img, nfeatures=nf))
    return out


# ---------------------------------------------------------------- e. orientation
def family_e(rng):
    w, h = 220, 160
    img = canvas(w, h)
    sites = [(x, y) for y in (30, 65, 100, 130) for x in (30, 65, 100, 135, 170)]
    # (du, dv, c) of low-contrast pixels (< minTh: no corners of their own) placed around a dot
    patterns = [
        [],                                            # point-symmetric: m10 = m01 = 0
        [(5, 5, 6), (-5, -5, 6)],                      # point-symmetric again
        [(0, 5, 6)], [(0, -5, 6)],                     # m10 = 0, m01 of both signs
        [(5, 0, 6)], [(-5, 0, 6)],                     # m01 = 0, m10 of both signs
        [(5, 5, 6)], [(-5, 5, 6)], [(5, -5, 6)], [(-5, -5, 6)],    # |m10| == |m01| in all four quadrants
        [(7, 3, 5), (3, 7, 5)], [(2, 6, 6), (6, 2, 6)],            # |m10| == |m01| from two pixels
        [(15, 1, 6)], [(-15, -1, 6)], [(1, 15, 6)], [(-1, -15, 6)],  # on the umax boundary (cvRound vs floor differ)
        [(14, 4, 6), (4, 14, 6)], [(11, 9, 6), (-9, -11, 6)],
        [(13, 7, 6)], [(10, 11, 6), (0, -15, 5)],
    ]
    for (x, y), pat in zip(sites, patterns):
        dot(img, x, y, 30)
        for du, dv, c in pat:
            dot(img, x + du, y + dv, c)
    return [case("e", "moments", img), case("e", "moments_dark", (255 - img).astype(np.uint8))]


# ---------------------------------------------------------------- f. blur and rBRIEF at the borders
def tie_row(img, y):
    """A row whose 7x7 column-pass sum sits exactly at the half in every column: rows y-2 .. y+2 at 129 126 128 126 129 on the
    128 canvas (sum K_i K_j p = 66049*128 + 257*(2*34 - 2*2*49) = 2^15 * 257, so (C + 2^15) >> 16 rounds 128.5).  The profile is
    symmetric about row y and constant along it: a keypoint on row y sees no moment from it."""
    for dy, d in ((-2, 1), (-1, -2), (1, -2), (2, 1)):
        img[y + dy, :] = BG + d


TAIL_TIE_COLUMNS = {2: (-3, 3, -2, -1), 3: (-2, -3, 1, 2)}     # found by search over the last four columns


def family_f(rng):
    out = []
    for (w, h) in ((214, 150), (215, 151), (216, 149)):        # w % 4 = 2, 3, 0
        img = canvas(w, h)
        band = rng.randint(0, 256, (h, w)).astype(np.uint8)
        img[:, :16] = band[:, :16]                             # textured border columns / rows: never tested by FAST (its
        img[:16, :] = band[:16, :]                             # ring stops at 16), read by IC_Angle and the blur of the
        img[h - 16:, :w - 24] = band[h - 16:, :w - 24]         # extreme taps
        yt = h // 2
        tie_row(img, yt)
        xs = (19, 20, 21, w - 27, w - 26, w - 20)
        ys = (19, 20, 21, h - 22, h - 21, h - 20)
        for k, x in enumerate(xs):
            dot(img, x, ys[k], 35)
            dot(img, x, ys[(k + 3) % 6], -35)
        dot(img, w - 20, yt, 30)                               # on the tie row, aimed at 45 degrees: the pattern's reach
        dot(img, w - 15, yt + 5, 6)                            # of 18 lands on tie pixels of the tail columns
        dot(img, 40, yt, 30)                                   # ... and of the vector columns
        dot(img, 45, yt + 5, 6)
        if w % 4:
            # columns w-4 .. w-1 (beyond IC_Angle's reach from w-20) whose 7x7 sums sit at the half in tail column w-2 (w % 4 = 2)
            # or w-3 (w % 4 = 3), on every row away from the tie row
            img[:, w - 4:] = BG + np.array(TAIL_TIE_COLUMNS[w % 4], np.int64)
        dot(img, w - 20, yt + 30, 30)                          # 45 degrees: taps (+18, -1) and (+17, -1) land in the tail
        dot(img, w - 15, yt + 35, 6)
        dot(img, w - 26, yt - 30, 30)                          # 315 degrees
        dot(img, w - 21, yt - 35, 6)
        for k in range(8):                                     # flat-area keypoints: t0 == t1 almost everywhere
            dot(img, 45 + 18 * k, 45 + (k % 3) * 14, 28)
        for tie in (0, 1):
            out.append(case("f", "borders_%dx%d_tie%d" % (w, h, tie), img.copy(), nfeatures=300, tie=tie))
    return out


# ---------------------------------------------------------------- g. levels and assembly
def family_g(rng):
    out = []
    w, h = 244, 180
    img = canvas(w, h)
    for k, (x, y) in enumerate(((60, 60), (120, 70), (180, 120), (80, 130))):
        img[y:y + 2, x:x + 2] = BG + 40 + 5 * k              # 2 x 2 blocks: plateaus on level 0, single corners further up
    img[40:43, 150:153] = BG - 45
    for (scale, nl) in ((1.2, 3), (2.0, 2)):
        out.append(case("g", "levels_s%.1f_n%d" % (scale, nl), img.copy(), nfeatures=120, scale=scale, nlevels=nl))
    img = canvas(w, h)
    for k in range(30):
        x, y = int(rng.randint(20, w - 24)), int(rng.randint(20, h - 24))
        img[y:y + 3, x:x + 3] = int(rng.choice([BG + 50, BG - 50]))
    out.append(case("g", "blocks_s1.2_n3", img, nfeatures=150, scale=1.2, nlevels=3))
    return out


# ---------------------------------------------------------------- h. extremes
def family_h(rng):
    w, h = 160, 124
    out = []
    img = (rng.randint(0, 2, (h // 4, w // 4)) * 255).astype(np.uint8).repeat(4, 0).repeat(4, 1)
    out.append(case("h", "binary_blocks", img, nfeatures=150, nlevels=2))
    img = (rng.randint(0, 2, (h, w)) * 255).astype(np.uint8)
    out.append(case("h", "binary_noise", img, nfeatures=150, nlevels=2))
    w, h = 212, 150
    img = np.zeros((h, w), np.uint8)
    for k in range(20):
        img[int(rng.randint(20, h - 20)), int(rng.randint(20, w - 20))] = 255
    out.append(case("h", "dots_255_on_0", img, nfeatures=100, scale=2.0, nlevels=2))
    out.append(case("h", "dots_0_on_255", (255 - img).astype(np.uint8), nfeatures=100, scale=2.0, nlevels=2))
    return out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g,
            "h": family_h}

TARGETS = {
    "a": ["fast_at_threshold", "retry", "retry_found", "retry_after_nms"],
    "b": ["nms_tie_orth", "nms_tie_diag", "nms_ring_kept", "score_saturated"],
    "c": ["cell_skip_x", "cell_skip_y", "cell_row_kept_in_x_skip_zone", "cell_clip_x", "cell_clip_y", "cell_short",
          "corner_first_col", "corner_last_col", "corner_first_row", "corner_last_row"],
    "d": ["order_not_raster", "node_tie", "octree_N_eq", "octree_N_plus1", "octree_N_minus1", "octree_roots",
          "octree_final_phase", "octree_equal_sizes"],
    "e": ["atan_zero", "atan_axis", "atan_diag", "umax_edge"],
    "f": ["blur_reflect_tap", "blur_tie_vec_tap", "blur_tie_tail_tap", "brief_equal"],
    "g": ["level_gt0_keypoint", "size_truncated", "pt_scaled_inexact"],
    "h": ["score_saturated", "nms_tie_orth"],
}


def fused_variant(case):
    """The case as the fused launch sees it: at least 2 levels (level 0 is then detected by the fused launch) and scale 1.2 (a
    scale factor the 4 x 4 resize takes)."""
    return dict(case, name=case["name"] + "_fused", nlevels=max(2, case["nlevels"]), scale=1.2)


def all_cases(seed=0, families="abcdefgh"):
    out = []
    for f in families:
        out.extend(FAMILIES[f](np.random.RandomState(seed * 131 + ord(f))))
    return out


def run_oracle(case, oracle):
    """(keypoints, descriptors, level images) of the oracle."""
    o = oracle.OrbOracle(case["nfeatures"], case["scale"], case["nlevels"], case["ini"], case["min"], blur_tie_mode=case["tie"])
    kps, desc = o.extract(case["img"])
    return kps, desc, [o.level_image(l) for l in range(case["nlevels"])]


def run_reference(case, levels, rules=None, hits=None):
    return R.extract(levels, case["nfeatures"], case["scale"], case["nlevels"], case["ini"], case["min"], case["tie"], rules, hits)


def same(a, b):
    return len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
