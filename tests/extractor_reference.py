"""A plain, sequential restatement of the ORB extractor after the pyramid, written from the upstream text
(thirdparty/orb-slam2/src/ORBextractor.cc) and the project's stated OpenCV 2.4 contract: it does not import oracle/, and apart
from the sin/cos sequence (below) it was not derived from the oracle's C or from the HIP kernels, so a misreading of
ORBextractor.cc shared by those two sides shows up as a disagreement here.

Scope: everything after ComputePyramid.  `extract` takes the level images as input -- the tests pass
OrbOracle.level_image(l) -- because the resize is pinned on its own (test_oracle.py: test_resize_vs_numpy,
test_resize_geometry_matches_torch_bilinear).  Covered: the cell loop of ComputeKeyPointsOctTree (:765-829), DistributeOctTree
(:539-763), the per-level quotas and scale factors (:415-439), IC_Angle with umax (:77-104, :452-469), GaussianBlur 7x7 sigma 2
REFLECT_101 (:1084-1085), computeOrbDescriptor (:107-147) and the output assembly (:831-846, :1094-1102).

Where upstream calls into OpenCV 2.4, the project's recalled contract is restated (PARITY UNPINNED):
- cv::FAST(img, kps, t, true): a pixel of rows / columns 3 .. n-4 is a corner when 9 contiguous pixels of its radius-3 ring
  are all brighter than p + t or all darker than p - t (strict); its score is the largest t for which that holds; NMS keeps a
  corner whose score is strictly greater than those of all 8 neighbours, the window's 3-px ring scoring 0; corners come out
  in the window's raster order;
- cv::fastAtan2: the published degree-7 polynomial in float, first branch when `ax >= ay`;
- cvRound: round half to even;
- GaussianBlur(7x7, 2, 2) on 8U: Q8 taps [18 34 49 55 49 34 18], a row pass then a column pass in integers, (sum + 2^15) >> 16;
  blur_tie_mode 0: a column-pass sum exactly at the half rounds to even in the vector columns x < (w & ~3) and up in the tail
  columns; blur_tie_mode 1: up everywhere;
- cos / sin of the keypoint angle: evaluated in double by the fixed sequence of the sin/cos contract and rounded once to float.
  DESIGN.md section 5 states the contract but not the sequence, so `contract_sincos` transcribes the oracle's orc_sincos_f
  constant for constant: this one primitive is NOT independently pinned (upstream calls the platform's cosf / sinf).

Every value upstream computes in `float` is an np.float32, evaluated in upstream's order.  `rules` (a Rules) switches one rule
to a wrong reading; the defaults are upstream's behaviour.  `hits` (a collections.Counter, or None) counts the edges a call
reached, so a test can assert that its case family really exercised the rule it targets.
"""
import math
import os
from dataclasses import dataclass

import numpy as np

f32 = np.float32
PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD = 31, 15, 19      # ORBextractor.cc:72-74
CELL_W = f32(30)                                              # const float W = 30 (:769)
BLUR_TAPS = (18, 34, 49, 55, 49, 34, 18)                      # Q8 taps of the 7x7 sigma-2 kernel
# cv::FAST's 16-pixel circle of radius 3 as (dx, dy), in ring order
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3))
HERE = os.path.dirname(os.path.abspath(__file__))
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


@dataclass(frozen=True)
class Rules:
    fast_decision: str = "gt"     # a ring pixel counts when beyond p + t strictly | "ge"
    nms: str = "gt"               # NMS keeps a corner strictly above its 8 neighbours | "ge"
    nms_scope: str = "window"     # scores visible only inside the cell window | "level": across the whole level
    retry: str = "cell"           # minThFAST retry per cell (:805-815) | "level": only when the whole level found nothing
    skip_x: int = 6               # iniX >= maxBorderX - 6 skips a column (:803) | 3
    order: str = "cell"           # candidates in (cell row, cell column, y, x) order | "raster": (y, x)
    node_keep: str = "first"      # DistributeOctTree keeps the first maximum of a node (:744-757) | "last"
    umax: str = "round"           # umax[v] = cvRound(sqrt(hp2 - v*v)) (:461-462) | "floor"
    atan_branch: str = "ge"       # fastAtan2's `ax >= ay` | "gt"
    blur_border: str = "reflect101"   # BORDER_REFLECT_101 (:1085) | "reflect"
    blur_tail: str = "split"      # half-to-even only for x < (w & ~3) | "uniform": the same rounding in every column
    brief_cmp: str = "lt"         # t0 < t1 (:125-141) | "le"
    size: str = "int"             # (int)(PATCH_SIZE * scale) (:831) | "float": no truncation


REFERENCE = Rules()
MUTANTS = {
    "fast_decision=ge": Rules(fast_decision="ge"),
    "nms=ge": Rules(nms="ge"),
    "nms_scope=level": Rules(nms_scope="level"),
    "retry=level": Rules(retry="level"),
    "skip_x=3": Rules(skip_x=3),
    "order=raster": Rules(order="raster"),
    "node_keep=last": Rules(node_keep="last"),
    "umax=floor": Rules(umax="floor"),
    "atan_branch=gt": Rules(atan_branch="gt"),
    "blur_border=reflect": Rules(blur_border="reflect"),
    "blur_tail=uniform": Rules(blur_tail="uniform"),
    "brief_cmp=le": Rules(brief_cmp="le"),
    "size=float": Rules(size="float"),
}


def _hit(hits, key, n=1):
    if hits is not None and n:
        hits[key] += n


def cv_round(v):
    """cvRound: half to even."""
    return int(np.rint(np.float64(v)))


def c_round(v):
    """C round(): half away from zero (DistributeOctTree's nIni, :543)."""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def pattern31():
    """bit_pattern_31_ (:150-408) as data: [256, 4] rows (x0, y0, x1, y1)."""
    txt = open(os.path.join(HERE, "..", "oracle", "orb_pattern31.inc")).read()
    vals = [int(v) for v in txt[txt.index("*/") + 2:].replace("\n", " ").split(",") if v.strip()]
    return np.array(vals, np.int64).reshape(256, 4)


# ---------------------------------------------------------------- constructor tables (:415-469)
def scale_factors(scale_factor, nlevels):
    """mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor: float times the double member, stored as float (:419-423)."""
    sf = [f32(1.0)]
    for _ in range(nlevels):
        sf.append(f32(np.float64(sf[-1]) * np.float64(f32(scale_factor))))
    return np.array(sf, np.float32)


def features_per_level(nfeatures, scale_factor, nlevels):
    """mnFeaturesPerLevel (:428-439): factor = 1.0f / scaleFactor (in double, stored as float), the series in float."""
    factor = f32(1.0 / np.float64(f32(scale_factor)))
    n_desired = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(math.pow(float(factor), float(nlevels)))))
    out, total = [], 0
    for _ in range(nlevels):
        out.append(cv_round(n_desired))
        total += out[-1]
        n_desired = f32(n_desired * factor)
    out.append(max(nfeatures - total, 0))
    return out


def umax_table(rules=None):
    """umax (:452-469): cvRound(sqrt(hp2 - v*v)) up to vmax, then the rows from vmin on mirrored so the disc is symmetric."""
    rules = rules or REFERENCE
    umax = [0] * (HALF_PATCH_SIZE + 1)
    vmax = int(math.floor(HALF_PATCH_SIZE * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(HALF_PATCH_SIZE * math.sqrt(2.0) / 2))
    hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
    for v in range(vmax + 1):
        r = math.sqrt(hp2 - v * v)
        umax[v] = int(math.floor(r)) if rules.umax == "floor" else cv_round(r)
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


# ---------------------------------------------------------------- FAST-9 (the cv::FAST contract)
def fast_arc_max_min(img):
    """For every pixel of rows / columns 3 .. n-4: the largest, over both polarities and all 16 arcs of 9 ring pixels, of the
    smallest contrast along the arc (0 elsewhere).  A pixel is a corner at threshold t when this exceeds t; its score is this - 1
    (the largest t that still makes it a corner)."""
    img = np.asarray(img, np.int64)
    h, w = img.shape
    out = np.zeros((h, w), np.int64)
    if h < 7 or w < 7:
        return out
    c = img[3:h - 3, 3:w - 3]
    ring = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    best = np.full(c.shape, -(1 << 20), np.int64)
    for d in (c[None] - ring, ring - c[None]):
        for k in range(16):
            best = np.maximum(best, d[[(k + j) % 16 for j in range(9)]].min(0))
    out[3:h - 3, 3:w - 3] = best
    return out


def _is_corner(M, t, rules):
    return M >= t if rules.fast_decision == "ge" else M > t


def fast_nms(M, t, rules=None, hits=None, level_scores=None, origin=(0, 0)):
    """cv::FAST(window, kps, t, true) on a window whose arc map is M: [(x, y, score)] in raster order, window coordinates.
    `level_scores` (the nms_scope=level mutant only): the level-wide score map NMS then compares against, the window at
    `origin` = (x0, y0)."""
    rules = rules or REFERENCE
    h, w = M.shape
    if h < 7 or w < 7:
        return []
    inner = np.zeros((h, w), bool)
    inner[3:h - 3, 3:w - 3] = True
    corner = inner & _is_corner(M, t, rules)
    score = np.where(corner, M - 1, 0)
    _hit(hits, "fast_at_threshold", int((inner & (M == t)).sum()))
    x0, y0 = origin
    out = []
    ys, xs = np.nonzero(corner)
    for y, x in zip(ys.tolist(), xs.tolist()):
        s = int(score[y, x])
        if s == 0:                                  # cannot beat a neighbour of score 0
            continue
        if s == 254:
            _hit(hits, "score_saturated")
        keep, tie_o, tie_d, hidden = True, False, False, False
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not (dx or dy):
                    continue
                n = int(score[y + dy, x + dx] if level_scores is None else level_scores[y0 + y + dy, x0 + x + dx])
                if n == s:
                    tie_d, tie_o = tie_d or bool(dx and dy), tie_o or not (dx and dy)
                if (n > s) if rules.nms == "ge" else (n >= s):
                    keep = False
                if not inner[y + dy, x + dx] and M[y + dy, x + dx] - 1 > s:
                    hidden = True                   # a stronger corner on the window's ring, which NMS cannot see
        _hit(hits, "nms_tie_orth", int(tie_o))
        _hit(hits, "nms_tie_diag", int(tie_d))
        if keep:
            _hit(hits, "nms_ring_kept", int(hidden))
            out.append((x, y, s))
    return out


# ---------------------------------------------------------------- ComputeKeyPointsOctTree's cell loop (:765-829)
def level_cells(w, h, rules=None, hits=None):
    """The FAST windows of a w x h level, in the loop's order: [(i, j, iniX, iniY, maxX, maxY, wCell, hCell)], and the borders
    (minBorderX, maxBorderX, minBorderY, maxBorderY)."""
    rules = rules or REFERENCE
    min_border_x = EDGE_THRESHOLD - 3
    min_border_y = min_border_x
    max_border_x = w - EDGE_THRESHOLD + 3
    max_border_y = h - EDGE_THRESHOLD + 3
    borders = (min_border_x, max_border_x, min_border_y, max_border_y)
    width = f32(max_border_x - min_border_x)
    height = f32(max_border_y - min_border_y)
    n_cols = int(f32(width / CELL_W))
    n_rows = int(f32(height / CELL_W))
    if n_cols <= 0 or n_rows <= 0:
        _hit(hits, "level_no_cells")
        return [], borders
    w_cell = int(math.ceil(f32(width / f32(n_cols))))
    h_cell = int(math.ceil(f32(height / f32(n_rows))))
    cells = []
    for i in range(n_rows):
        ini_y = f32(min_border_y + i * h_cell)
        max_y = f32(ini_y + f32(h_cell + 6))
        if ini_y >= max_border_y - 3:
            _hit(hits, "cell_skip_y")
            continue
        if ini_y >= max_border_y - 6:
            _hit(hits, "cell_row_kept_in_x_skip_zone")
        if max_y > max_border_y:
            _hit(hits, "cell_clip_y")
            max_y = f32(max_border_y)
        for j in range(n_cols):
            ini_x = f32(min_border_x + j * w_cell)
            max_x = f32(ini_x + f32(w_cell + 6))
            if ini_x >= max_border_x - rules.skip_x:
                _hit(hits, "cell_skip_x")
                continue
            if max_x > max_border_x:
                _hit(hits, "cell_clip_x")
                max_x = f32(max_border_x)
            if int(max_x) - int(ini_x) < 7 or int(max_y) - int(ini_y) < 7:
                _hit(hits, "cell_short")
            cells.append((i, j, int(ini_x), int(ini_y), int(max_x), int(max_y), w_cell, h_cell))
    return cells, borders


def level_candidates(img, ini_th, min_th, rules=None, hits=None):
    """vToDistributeKeys of one level: [(x, y, response)] with x, y relative to (minBorderX, minBorderY), in the order upstream
    pushes them (cell row, cell column, then the window's raster order); and the borders."""
    rules = rules or REFERENCE
    h, w = img.shape
    M = fast_arc_max_min(img)
    cells, borders = level_cells(w, h, rules, hits)

    def detect(c, t):
        _, _, x0, y0, x1, y1, _, _ = c
        level_scores = np.where(_is_corner(M, t, rules), M - 1, 0) if rules.nms_scope == "level" else None
        return fast_nms(M[y0:y1, x0:x1], t, rules, hits, level_scores, (x0, y0))

    found = []
    for c in cells:
        keys = detect(c, ini_th)
        if not keys and rules.retry == "cell":
            _hit(hits, "retry")
            _, _, x0, y0, x1, y1, _, _ = c
            win = M[y0:y1, x0:x1]
            if win.shape[0] >= 7 and win.shape[1] >= 7 and np.any(_is_corner(win[3:-3, 3:-3], ini_th, rules)):
                _hit(hits, "retry_after_nms")          # corners at iniThFAST, none left after NMS
            keys = detect(c, min_th)
            _hit(hits, "retry_found", int(bool(keys)))
        found.append((c, keys))
    if rules.retry == "level" and not any(k for _, k in found):
        found = [(c, detect(c, min_th)) for c in cells]
    cand = []
    for (i, j, x0, y0, x1, y1, w_cell, h_cell), keys in found:
        for (x, y, s) in keys:
            cand.append((x + j * w_cell, y + i * h_cell, s))     # pt += (j*wCell, i*hCell) (:817-821)
            ax, ay = x0 + x, y0 + y
            _hit(hits, "corner_first_col", int(ax == borders[0] + 3))
            _hit(hits, "corner_last_col", int(ax == borders[1] - 4))
            _hit(hits, "corner_first_row", int(ay == borders[2] + 3))
            _hit(hits, "corner_last_row", int(ay == borders[3] - 4))
    raster = sorted(cand, key=lambda k: (k[1], k[0]))
    _hit(hits, "order_not_raster", int(raster != cand))
    if rules.order == "raster":
        cand = raster
    return cand, borders


# ---------------------------------------------------------------- DistributeOctTree (:539-763)
def distribute_octtree(cand, min_x, max_x, min_y, max_y, n_target, rules=None, hits=None):
    """Indices into `cand` ([(x, y, response)], relative to (minX, minY)) of the keypoints DistributeOctTree returns, in its
    output order (the node list from front to back).  The sort of vPrevSizeAndPointerToNode compares (size, node address);
    for equal sizes the project's parity contract takes the later created node first."""
    rules = rules or REFERENCE
    n_ini = c_round(f32(f32(max_x - min_x) / f32(max_y - min_y)))
    h_x = f32(f32(max_x - min_x) / f32(n_ini))
    _hit(hits, "octree_roots", int(n_ini > 1))
    seq = [0]

    def node(ulx, uly, urx, bry, keys):
        seq[0] += 1
        return {"b": (ulx, uly, urx, bry), "k": keys, "s": seq[0], "nomore": len(keys) == 1}

    roots = [node(int(f32(h_x * f32(i))), 0, int(f32(h_x * f32(i + 1))), max_y - min_y, []) for i in range(n_ini)]
    for i, (x, y, r) in enumerate(cand):
        roots[int(f32(f32(x) / h_x))]["k"].append(i)
    nodes = [n for n in roots if n["k"]]
    for n in nodes:
        n["nomore"] = len(n["k"]) == 1

    def divide(n):
        ulx, uly, urx, bry = n["b"]
        hx = int(math.ceil(f32(f32(urx - ulx) / f32(2))))
        hy = int(math.ceil(f32(f32(bry - uly) / f32(2))))
        mx, my = ulx + hx, uly + hy
        ks = [[], [], [], []]
        for i in n["k"]:
            x, y, _ = cand[i]
            ks[(0 if y < my else 2) if x < mx else (1 if y < my else 3)].append(i)
        bs = [(ulx, uly, mx, my), (mx, uly, urx, my), (ulx, my, mx, bry), (mx, my, urx, bry)]
        return [node(*bs[q], ks[q]) for q in range(4)]

    finish = False
    while not finish:
        prev = len(nodes)
        vec, n_expand, front = [], 0, []
        for n in list(nodes):
            if n["nomore"]:
                continue
            for ch in divide(n):                     # children pushed to the FRONT of the list, n1 first (:621-662)
                if ch["k"]:
                    front.insert(0, ch)
                    if len(ch["k"]) > 1:
                        n_expand += 1
                        vec.append(ch)
            nodes.remove(n)
        nodes = front + nodes
        if len(nodes) >= n_target or len(nodes) == prev:
            finish = True
        elif len(nodes) + 3 * n_expand > n_target:
            _hit(hits, "octree_final_phase")
            while not finish:
                prev = len(nodes)
                sizes = [len(n["k"]) for n in vec]
                _hit(hits, "octree_equal_sizes", int(len(sizes) != len(set(sizes))))
                pv = sorted(vec, key=lambda n: (len(n["k"]), n["s"]))
                vec = []
                for n in reversed(pv):
                    for ch in divide(n):
                        if ch["k"]:
                            nodes.insert(0, ch)
                            if len(ch["k"]) > 1:
                                vec.append(ch)
                    nodes.remove(n)
                    if len(nodes) >= n_target:
                        break
                if len(nodes) >= n_target or len(nodes) == prev:
                    finish = True
    out = []
    for n in nodes:
        best = n["k"][0]
        for i in n["k"][1:]:
            r, rb = cand[i][2], cand[best][2]
            _hit(hits, "node_tie", int(r == rb))
            if r > rb or (rules.node_keep == "last" and r == rb):
                best = i
        out.append(best)
    return out


# ---------------------------------------------------------------- fastAtan2 and IC_Angle (:77-104)
_RAD2DEG = f32(180.0 / math.pi)
ATAN2_P = [f32(f32(c) * _RAD2DEG) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
                                             -0.04432655554792128)]
_DBL_EPS_F = f32(2.220446049250313e-16)                       # (float)DBL_EPSILON


def fast_atan2(y, x, rules=None, hits=None):
    """cv::fastAtan2 in degrees, [0, 360)."""
    rules = rules or REFERENCE
    y, x = f32(y), f32(x)
    ax, ay = abs(x), abs(y)
    p1, p3, p5, p7 = ATAN2_P
    if ax == ay:
        _hit(hits, "atan_zero" if ax == 0 else "atan_diag")
    elif ax == 0 or ay == 0:
        _hit(hits, "atan_axis")
    first = (ax > ay) if rules.atan_branch == "gt" else (ax >= ay)
    c = f32(ay / f32(ax + _DBL_EPS_F)) if first else f32(ax / f32(ay + _DBL_EPS_F))
    c2 = f32(c * c)
    poly = f32(f32(f32(f32(f32(f32(f32(p7 * c2) + p5) * c2) + p3) * c2) + p1) * c)
    a = poly if first else f32(f32(90.0) - poly)
    if x < 0:
        a = f32(f32(180.0) - a)
    if y < 0:
        a = f32(f32(360.0) - a)
    return a


def ic_moments(img, x, y, umax):
    """(m_10, m_01) of the circular patch at integer (x, y): the centre row, then rows +-v up to umax[v] (:79-101)."""
    I = np.asarray(img, np.int64)
    us = np.arange(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1)
    m10 = int((us * I[y, x - HALF_PATCH_SIZE:x + HALF_PATCH_SIZE + 1]).sum())
    m01 = 0
    for v in range(1, HALF_PATCH_SIZE + 1):
        d = umax[v]
        us = np.arange(-d, d + 1)
        plus, minus = I[y + v, x - d:x + d + 1], I[y - v, x - d:x + d + 1]
        m10 += int((us * (plus + minus)).sum())
        m01 += v * int((plus - minus).sum())
    return m10, m01


# ---------------------------------------------------------------- GaussianBlur 7x7 sigma 2 (contract) and rBRIEF (:107-147)
def gaussian_blur7(img, tie_mode=0, rules=None):
    """(blurred, tie): tie marks the pixels whose column-pass sum sat exactly at the half."""
    rules = rules or REFERENCE
    h, w = img.shape
    K = np.array(BLUR_TAPS, np.int64)
    # numpy's "reflect" is BORDER_REFLECT_101 (gfedcb|abcdefgh), "symmetric" is BORDER_REFLECT (fedcba|abcdefgh)
    p = np.pad(np.asarray(img, np.int64), 3, mode="symmetric" if rules.blur_border == "reflect" else "reflect")
    R = sum(K[i] * p[:, i:i + w] for i in range(7))
    C = sum(K[i] * R[i:i + h, :] for i in range(7))
    v = (C + 32768) >> 16
    tie = (C & 0xFFFF) == 0x8000
    if tie_mode == 0:
        even = np.arange(w)[None, :] < (w if rules.blur_tail == "uniform" else (w & ~3))
        v = np.where(tie & even, v & ~1, v)
    return np.minimum(v, 255).astype(np.uint8), tie


def contract_sincos(angle):
    """(sin, cos) of a float angle in radians by the project's sin/cos contract: Cody-Waite reduction by pi/2 in double, Taylor
    polynomials to degree 17 / 18 in double without fused multiply-adds, one rounding to float.  Transcribed from the oracle's
    orc_sincos_f (the contract's only statement of the sequence), so not an independent check of it."""
    x = float(f32(angle))
    k = math.floor(x * 0.63661977236758138243 + 0.5)
    r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11
    r2 = r * r
    ps = -1.0 / 355687428096000.0
    for c in (1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0,
              1.0 / 6.0):
        ps = ps * r2 + c
    sn = r - (r * r2) * ps
    pc = -1.0 / 6402373705728000.0
    for c in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0,
              -1.0 / 720.0, 1.0 / 24.0, -0.5):
        pc = pc * r2 + c
    cs = 1.0 + r2 * pc
    s, c = ((sn, cs), (cs, -sn), (-sn, -cs), (-cs, sn))[int(k) & 3]
    return f32(s), f32(c)


FACTOR_PI = f32(math.pi / np.float64(f32(180.0)))           # (float)(CV_PI/180.f) (:107)
_PATTERN = []


def orb_descriptor(blurred, x, y, angle_deg, rules=None, hits=None, tie=None):
    """computeOrbDescriptor at integer (x, y) of the blurred level: 256 tests t0 < t1, bit k of byte i from pair 8i + k."""
    rules = rules or REFERENCE
    if not _PATTERN:
        _PATTERN.append(pattern31())
    pat = _PATTERN[0]
    angle = f32(f32(angle_deg) * FACTOR_PI)
    b, a = contract_sincos(angle)                            # a = cos(angle), b = sin(angle) (:112)
    px = pat[:, 0::2].astype(np.float32)
    py = pat[:, 1::2].astype(np.float32)
    # GET_VALUE: row cvRound(x*b + y*a), column cvRound(x*a - y*b), each product and the sum rounded to float (:118-119)
    ry = np.rint((px * b + py * a).astype(np.float32).astype(np.float64)).astype(np.int64)
    rx = np.rint((px * a - py * b).astype(np.float32).astype(np.float64)).astype(np.int64)
    ty, tx = y + ry, x + rx
    B = np.asarray(blurred, np.int64)
    vals = B[ty, tx]
    t0, t1 = vals[:, 0], vals[:, 1]
    if hits is not None:
        h, w = B.shape
        _hit(hits, "brief_equal", int((t0 == t1).sum()))
        _hit(hits, "blur_reflect_tap", int(((tx < 3) | (tx >= w - 3) | (ty < 3) | (ty >= h - 3)).sum()))
        if tie is not None:
            t = tie[ty, tx]
            _hit(hits, "blur_tie_vec_tap", int((t & (tx < (w & ~3))).sum()))
            _hit(hits, "blur_tie_tail_tap", int((t & (tx >= (w & ~3))).sum()))
    bits = (t0 <= t1) if rules.brief_cmp == "le" else (t0 < t1)
    return np.packbits(bits.astype(np.uint8), bitorder="little")


# ---------------------------------------------------------------- ORBextractor::operator() after ComputePyramid
def extract(levels, nfeatures, scale_factor, nlevels, ini_th, min_th, blur_tie_mode=0, rules=None, hits=None):
    """(keypoints KEYPOINT_DTYPE, descriptors [n, 32] uint8) from the nlevels level images, levels in order, each level's
    keypoints in DistributeOctTree's output order (:1073-1102)."""
    rules = rules or REFERENCE
    sf = scale_factors(scale_factor, nlevels)
    quota = features_per_level(nfeatures, scale_factor, nlevels)
    umax = umax_table(rules)
    umax_floor = umax_table(Rules(umax="floor"))
    kps_all, desc_all = [], []
    for level in range(nlevels):
        img = np.asarray(levels[level], np.uint8)
        cand, (bx0, bx1, by0, by1) = level_candidates(img, ini_th, min_th, rules, hits)
        if not cand:
            continue
        n, q = len(cand), quota[level]
        _hit(hits, {0: "octree_N_eq", 1: "octree_N_plus1", -1: "octree_N_minus1"}.get(n - q, "octree_N_other"))
        keep = distribute_octtree(cand, bx0, bx1, by0, by1, q, rules, hits)
        # const int scaledPatchSize = PATCH_SIZE*mvScaleFactor[level] (:831): int * float, truncated to int
        scaled = f32(f32(PATCH_SIZE) * sf[level])
        size = f32(int(scaled)) if rules.size == "int" else scaled
        _hit(hits, "size_truncated", int(f32(int(scaled)) != scaled))
        blurred, tie = gaussian_blur7(img, blur_tie_mode, rules)
        kps = np.zeros(len(keep), KEYPOINT_DTYPE)
        desc = np.zeros((len(keep), 32), np.uint8)
        for k, ci in enumerate(keep):
            x, y, r = cand[ci]
            x, y = x + bx0, y + by0                         # pt += (minBorderX, minBorderY) (:836-843)
            m10, m01 = ic_moments(img, x, y, umax)
            if hits is not None and ic_moments(img, x, y, umax_floor) != (m10, m01):
                _hit(hits, "umax_edge")
            angle = fast_atan2(f32(m01), f32(m10), rules, hits)
            desc[k] = orb_descriptor(blurred, x, y, angle, rules, hits, tie)
            if level:
                _hit(hits, "level_gt0_keypoint")
                px, py = f32(f32(x) * sf[level]), f32(f32(y) * sf[level])     # pt *= scale, in float (:1094-1100)
                _hit(hits, "pt_scaled_inexact", int(float(px) != x * float(sf[level])))
            else:
                px, py = f32(x), f32(y)
            kps[k] = (px, py, size, angle, f32(r), level, -1)
        kps_all.append(kps)
        desc_all.append(desc)
    if not kps_all:
        return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    return np.concatenate(kps_all), np.concatenate(desc_all)
