// plan.hip -- the plan of one frame size: level geometry and the host tables of K1 (resize, fused), K2 (cells) and K3 (quadtree).
// Mirrors the host logic of ORB_SLAM2::ORBextractor that depends on the frame size:
//   level sizes             thirdparty/orb-slam2/src/ORBextractor.cc:1110-1111
//   cell grid               ORBextractor.cc:773-787
//   quadtree roots          ORBextractor.cc:543-545
// The builders make no HIP call: make_plan allocates, uploads what they return and resolves the device pointers.
#include "pgorb_ctx.h"

static inline int cvRound(double v) { return (int)lrint(v); }
static inline int cvFloor(double v) { int i = (int)v; return i - (v < i); }

int level_geometry(const pgorb_ctx* c, int w, int h, LevelGeom* g)
{
    for (int l = 0; l < c->prm.nlevels; l++) {
        const float scale = c->mvInvScaleFactor[l];                                // level sizes, :1110-1111
        g[l].w = cvRound((double)((float)w * scale)); g[l].h = cvRound((double)((float)h * scale));
        const float width = (float)(g[l].w - 2 * PG_EDGE), height = (float)(g[l].h - 2 * PG_EDGE);
        const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);     // :784-785
        if (nCols < 1 || nRows < 1) return PGORB_E_TOOSMALL;
        g[l].nCols = nCols; g[l].nRows = nRows;
        g[l].wCell = (int)ceilf(width / nCols);                                   // :786-787
        g[l].hCell = (int)ceilf(height / nRows);
        const int rw = g[l].w - 2 * PG_EDGE, rh = g[l].h - 2 * PG_EDGE;
        g[l].nIni = (int)roundf((float)rw / rh);                                  // :543
        // nIni == 0 (region more than twice as tall as wide): the reference divides by it and then
        // indexes an empty vector -- but only when the level has candidates (:545-570); with none it
        // returns an empty level.  Same here: K3 raises PGORB_E_TOOSMALL iff such a level has candidates.
        if (g[l].nIni < 1) g[l].nIni = 0;
        g[l].hX = g[l].nIni ? (float)rw / g[l].nIni : 0.f;                        // :545
    }
    return 0;
}

namespace {

// cv::resize INTER_LINEAR coefficient set-up for 8U (OpenCV 2.4 imgwarp.cpp; Appendix A1)
void build_resize_tables(int sw, int sh, int dw, int dh, std::vector<int32_t>& xofs,
                         std::vector<int32_t>& xofs1, std::vector<int16_t>& xalpha,
                         std::vector<int32_t>& yofs, std::vector<int16_t>& ybeta)
{
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    xofs.resize(dw); xofs1.resize(dw); xalpha.resize(2 * dw); yofs.resize(2 * dh); ybeta.resize(2 * dh);
    auto sat16 = [](int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); };
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cvFloor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }          // single-tap columns (dx >= xmax)
        xofs[dx] = sx;
        xofs1[dx] = sx + 1 < sw ? sx + 1 : sw - 1;
        xalpha[2 * dx] = sat16(cvRound((double)((1.f - fx) * 2048)));
        xalpha[2 * dx + 1] = sat16(cvRound((double)(fx * 2048)));
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cvFloor(fy);
        fy -= sy;
        int r0 = sy, r1 = sy + 1;
        r0 = r0 < 0 ? 0 : (r0 >= sh ? sh - 1 : r0);
        r1 = r1 < 0 ? 0 : (r1 >= sh ? sh - 1 : r1);
        yofs[2 * dy] = r0; yofs[2 * dy + 1] = r1;
        ybeta[2 * dy] = sat16(cvRound((double)((1.f - fy) * 2048)));
        ybeta[2 * dy + 1] = sat16(cvRound((double)(fy * 2048)));
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the resize tables of level l from level l - 1 (S the source level, D the level itself)
struct ResizeTabs {
    std::vector<int32_t> xofs, xofs1, yofs, tilex;
    std::vector<int16_t> xalpha, ybeta;
    std::vector<PgQuadTab> qt;
    std::vector<PgQuadTab2> q2;
    std::vector<uint8_t> yrel;
    std::vector<PgRowGrp> rg;
    bool hasQ = false, hasQ2 = false, hasY = false;
    int cpr = 0, prows = 0;                                           // LDS-staged form: 16-byte chunks per row, staged rows (0: does not fit)
};

ResizeTabs build_resize_level(const LevelGeom& S, const LevelGeom& D, int pyrGpw)
{
    ResizeTabs R;
    build_resize_tables(S.w, S.h, D.w, D.h, R.xofs, R.xofs1, R.xalpha, R.yofs, R.ybeta);
    const std::vector<int32_t>& xo = R.xofs; const std::vector<int32_t>& xo1 = R.xofs1; const std::vector<int32_t>& yo = R.yofs;
    const std::vector<int16_t>& xa = R.xalpha; const std::vector<int16_t>& yb = R.ybeta;
    // quad table for the fast path
    const int nq = (D.w + 3) / 4;
    std::vector<PgQuadTab>& qt = R.qt;
    qt.resize(nq);
    bool ok = true;
    for (int q = 0; q < nq; q++) {
        PgQuadTab& T = qt[q];
        memset(&T, 0, sizeof(T));
        T.base_dw = xo[4 * q] >> 2;
        for (int k = 0; k < 4; k++) {
            const int dx = 4 * q + k;
            if (dx >= D.w) break;
            const int o = xo[dx] - 4 * T.base_dw;
            if (o < 0 || o > 8) ok = false;
            // tap 1 is read at o+1; where cv::resize clamps it (xofs1 == xofs) its weight is 0
            if (xo1[dx] != xo[dx] + 1 && xa[2 * dx + 1] != 0) ok = false;
            T.offs |= (uint32_t)(o & 15) << (4 * k);
            T.a0[k] = xa[2 * dx]; T.a1[k] = xa[2 * dx + 1];
        }
    }
    R.hasQ = ok;
    // 8-byte-window table: xb = first tap of the quad (clamped so the window stays inside the row)
    std::vector<PgQuadTab2>& q2 = R.q2;
    q2.resize(nq);
    bool ok2 = S.w >= 8;
    for (int q = 0; q < nq && ok2; q++) {
        PgQuadTab2& T = q2[q];
        memset(&T, 0, sizeof(T));
        T.xb = std::min(xo[4 * q], S.w - 8);
        for (int k = 0; k < 4; k++) {
            const int dx = 4 * q + k;
            if (dx >= D.w) { T.sel[k] = 0x0c0c0c0cu; continue; }
            const int o0 = xo[dx] - T.xb, o1 = xo1[dx] - T.xb;
            if (o0 < 0 || o0 > 7 || o1 < 0 || o1 > 7) { ok2 = false; break; }
            T.sel[k] = (uint32_t)o0 | (0x0cu << 8) | ((uint32_t)o1 << 16) | (0x0cu << 24);
            T.coef[k] = (uint32_t)(uint16_t)xa[2 * dx] | ((uint32_t)(uint16_t)xa[2 * dx + 1] << 16);
            if (xa[2 * dx] < 0 || xa[2 * dx + 1] < 0) ok2 = false;
        }
    }
    R.hasQ2 = ok2;
    // row pattern for the 4-rows-per-lane kernel: r0(dy) - r0(group base) - d in {0,1}, r1 - r0 in {0,1}
    std::vector<uint8_t>& yr = R.yrel;
    yr.assign(D.h, 0);
    bool oky = true;
    for (int dy = 0; dy < D.h; dy++) {
        const int base = yo[2 * (dy & ~3)], d = dy & 3;
        const int e0 = yo[2 * dy] - base - d, e1 = yo[2 * dy + 1] - yo[2 * dy];
        if (e0 < 0 || e0 > 1 || e1 < 0 || e1 > 1) oky = false;
        yr[dy] = (uint8_t)((e0 & 1) | ((e1 & 1) << 1));
    }
    R.hasY = oky;
    std::vector<PgRowGrp>& rg = R.rg;
    rg.resize((D.h + 3) / 4 + 4);                                     // + records of slack (a wave loads its 1, 2 or 4 records at once)
    for (size_t gi = 0; gi < rg.size(); gi++) {
        PgRowGrp& G = rg[gi];
        memset(&G, 0, sizeof(G));
        G.sFirst = yo[2 * std::min((int)(4 * gi), D.h - 1)];
        for (int d = 0; d < 4; d++) {
            const int dy = std::min((int)(4 * gi) + d, D.h - 1);
            G.yrel4 |= (uint32_t)yr[dy] << (8 * d);
            G.ybeta[2 * d] = yb[2 * dy]; G.ybeta[2 * d + 1] = yb[2 * dy + 1];
        }
    }
    // LDS-staged variant of the 4x4 kernel: a 256 x 32 destination tile stages its source
    // rectangle (16-byte chunks from a 16-aligned first column) through LDS
    const int tileRows = 16 * pyrGpw, gpt = 4 * pyrGpw;               // rows / 4-row groups per tile
    const int ntx = (D.w + 255) / 256, nty = (D.h + tileRows - 1) / tileRows, ngrp = (D.h + 3) / 4;
    std::vector<int32_t>& tx0 = R.tilex;
    tx0.assign(ntx, 0);
    int span = 0, rows = 0;
    if (ok2 && oky) {
        for (int tx = 0; tx < ntx; tx++) {
            const int qf = 64 * tx, ql = std::min(64 * tx + 63, nq - 1);
            tx0[tx] = q2[qf].xb & ~15;
            span = std::max(span, q2[ql].xb + 8 - tx0[tx]);
        }
        for (int ty = 0; ty < nty; ty++) {
            const int gf = gpt * ty, gl = std::min(gpt * ty + gpt - 1, ngrp - 1);
            rows = std::max(rows, rg[gl].sFirst + 6 - rg[gf].sFirst);
        }
        const int cpr = (span + 4 + 15) / 16;
        if (cpr <= 32 && (size_t)rows * cpr * 16 <= (size_t)10 * 1024 * pyrGpw) { R.cpr = cpr; R.prows = rows; }
    }
    return R;
}

// the fused launch's tables with S as the source level (D the next level, R its resize tables); nb == 0: the level takes K1 + K2
struct FusedTabs {
    std::vector<int32_t> bands, cols;
    int nb = 0, spb = 0, rows = 0;
};

FusedTabs build_fused_level(const LevelGeom& S, const LevelGeom& D, const ResizeTabs& R)
{
    // fused resize + detect (fused.hip) with level l - 1 as the source: bands = the source level's cell rows (hCell + 6 staged
    // rows from row 16 + i hCell) between an edge band above (rows 0 ...) and below; a band owns the 4-row groups of level l whose
    // first source row lies in [its first row, the next band's first row), so that the six source rows of every group are staged;
    // tile columns = NS cells, a column owns the quads whose window starts in [15 + first cell * wCell, ... of the next column).
    FusedTabs F;
    const std::vector<PgQuadTab2>& q2 = R.q2;
    const std::vector<PgRowGrp>& rg = R.rg;
    const int nq = (int)q2.size();
    const int ngrp = (D.h + 3) / 4, rowsB = S.hCell + 6;
    bool fok = R.hasQ2 && R.hasY && S.wCell <= 32 && S.hCell <= 40 && S.hCell >= 16 && S.wCell >= 16;       // (the detector's narrow form; 3 x 21 staged rows)
    std::vector<int32_t> bands, cols;
    int nb = 0;
    if (fok) {
        const int maxS = rg[ngrp - 1].sFirst;
        std::vector<int> Y{0};
        for (int i = 0; i < S.nRows || PG_EDGE + i * S.hCell <= maxS; i++) Y.push_back(PG_EDGE + i * S.hCell);
        int gi = 0;
        for (size_t b = 0; b < Y.size(); b++) {
            const int yNext = b + 1 < Y.size() ? Y[b + 1] : INT32_MAX;
            const int g0 = gi;
            while (gi < ngrp && rg[gi].sFirst < yNext) {
                if (rg[gi].sFirst < Y[b] || rg[gi].sFirst + 5 - Y[b] > rowsB - 1) fok = false;
                gi++;
            }
            bands.insert(bands.end(), {g0, gi - g0});          // (the kernel derives the band's first row and cell row from b)
            nb++;
        }
        if (gi != ngrp) fok = false;
    }
    int spbF = 0;
    if (fok) {
        // slot columns: s = -1 the left edge's pseudo-cell (source columns from 0), s >= 0 from column 15 + s wCell (the cell's
        // iniX - 1; past the last cell column: pseudo-cells that only serve the resize); a quad belongs to the column its
        // 8-byte window starts in -- and then lies inside that column's 48 bytes
        auto slotOf = [&](int xb) { return xb < PG_EDGE - 1 ? -1 : (xb - (PG_EDGE - 1)) / S.wCell; };
        auto slotX = [&](int sl) { return sl < 0 ? 0 : PG_EDGE - 1 + sl * S.wCell; };
        int nSlotsTotal = S.nCols;
        for (int q = 0; q < nq; q++) {
            const int sl = slotOf(q2[q].xb), off = q2[q].xb - slotX(sl);
            if (q > 0 && q2[q].xb < q2[q - 1].xb) fok = false;
            if (off < 0 || (off & ~3) + 12 > 48) fok = false;
            nSlotsTotal = std::max(nSlotsTotal, sl + 1);
        }
        spbF = nSlotsTotal + 1;
        int qi = 0, maxNq = 0, maxNg = 0;
        for (int sl = -1; sl < nSlotsTotal; sl++) {
            const int q0 = qi;
            while (qi < nq && slotOf(q2[qi].xb) <= sl) qi++;
            const int n = qi - q0, magic = n > 0 ? 65536 / n + 1 : 65536;
            for (int lane = 0; lane < 64 && n > 0; lane++) if (((lane * magic) >> 16) != lane / n) fok = false;
            maxNq = std::max(maxNq, n);
            cols.insert(cols.end(), {q0, n, magic, 0});
        }
        if (qi != nq) fok = false;
        for (int b = 0; b < nb; b++) maxNg = std::max(maxNg, bands[2 * b + 1]);
        if (maxNq * maxNg > 64) fok = false;                   // lane = (quad, group)
    }
    if (fok) {
        F.bands = std::move(bands); F.cols = std::move(cols);
        F.nb = nb; F.spb = spbF; F.rows = rowsB;
    }
    return F;
}

// the per-frame sizes of the arenas and where every level starts in them
struct PlanLayout {
    size_t pyrOff[PG_MAXL];
    size_t pyrFrame = 0, candFrame = 0, selFrame = 0, nodeFrame = 0, cellCandFrame = 0;
    int cells = 0, selTotal = 0;
};

// Caps, slab offsets and node placement of every level into P.lvl, and the limits of the kernels (PGORB_E_LIMIT).
int build_layout(pgorb_ctx* c, const LevelGeom* g, PgPlan& P, PlanLayout& A)
{
    for (int l = 0; l < P.nlevels; l++) {
        PgLevel& V = P.lvl[l];
        V.w = g[l].w; V.h = g[l].h;
        V.pitch = (int)align_up(V.w, 64);
        V.fstride = (int64_t)align_up((size_t)V.pitch * V.h + 64, 256);
        A.pyrOff[l] = A.pyrFrame;
        A.pyrFrame += (size_t)V.fstride;
        V.nCols = g[l].nCols; V.nRows = g[l].nRows; V.wCell = g[l].wCell; V.hCell = g[l].hCell;
        V.cellBase = A.cells; A.cells += V.nCols * V.nRows;
        V.quota = c->mnFeaturesPerLevel[l];
        V.nIni = g[l].nIni; V.hX = g[l].hX;
        V.selCap = std::max(V.quota + 2, 4 * V.nIni);
        V.nodeCap = (int)align_up(V.selCap + 8, 4);
        // NMS survivors are never 8-adjacent: at most ceil(IW/2)*ceil(IH/2) per cell
        V.candCap = ((V.w - 2 * PG_EDGE) / 2 + V.nCols + 1) * ((V.h - 2 * PG_EDGE) / 2 + V.nRows + 1);
        V.candOff = (int64_t)A.candFrame; A.candFrame += align_up(V.candCap, 64);
        V.cellCap = ((V.wCell + 1) / 2) * ((V.hCell + 1) / 2);
        V.cellCandOff = (int64_t)A.cellCandFrame;
        A.cellCandFrame += align_up((size_t)V.cellCap * V.nCols * V.nRows, 64);
        V.selOff = (int64_t)A.selFrame; A.selFrame += V.selCap;      // slab offset == capacity prefix: K4-6's slot s of a frame IS entry s
        // node arrays of the quadtree: LDS when 30 ints per node fit its 140 KB, else a global slab
        // (quotas above ~1180 keypoints on one level: slower, but no configuration is refused)
        V.nodeOff = -1;
        // K3 keeps a level's node arrays (28 ints per node) in LDS beside its count pyramid (17 KB static) and its aux area
        // (max(pyramid leaves <= 3072, cells of the largest level + 1) ints); what does not fit 160 KB goes to a global slab
        const size_t qtAux = std::max((size_t)3072, (size_t)g[0].nCols * g[0].nRows + 1);
        const size_t qtTab = (size_t)2 * ((g[0].w - 2 * PG_EDGE) + (g[0].h - 2 * PG_EDGE));      // the prologue's coordinate tables share the node area
        if (std::max((size_t)V.nodeCap * 28, qtTab) * sizeof(int) + qtAux * sizeof(int) + 17 * 1024 > 160 * 1024) {
            V.nodeOff = (int64_t)A.nodeFrame;
            A.nodeFrame += align_up((size_t)V.nodeCap * 30, 64);
        }
        V.scale = c->mvScaleFactor[l];
        V.patchSize = (float)(int)(31 * c->mvScaleFactor[l]);                     // :836
        A.selTotal += V.selCap;
        if ((size_t)(V.nCols * V.nRows + 1) * sizeof(int) > 140 * 1024)
            return fail(c, PGORB_E_LIMIT, "too many cells on one level for the quadtree kernel's LDS budget");
        if (V.w > 4095 + 2 * PG_EDGE || V.h > 4095 + 2 * PG_EDGE)
            return fail(c, PGORB_E_LIMIT, "level larger than 4095 px is not supported");
        if (V.selCap > 65535)      // K3's dispatch-order sort packs a keypoint's arrival index into 16 bits
            return fail(c, PGORB_E_LIMIT, "more than 65533 keypoints on one pyramid level are not supported");
    }
    A.selFrame = align_up(A.selFrame, 16);
    P.totalCells = A.cells; P.selTotal = A.selTotal;
    P.cellCandFrame = (int64_t)A.cellCandFrame;
    P.candFrame = (int64_t)A.candFrame; P.selFrame = (int64_t)A.selFrame; P.nodeFrame = (int64_t)A.nodeFrame;
    return 0;
}

// K2's 64-byte cell records (PgPlan::cellTab) of a batch of B frames, and the same records in K2's balanced order
// (PgPlan::cellTabBal, `per` records per XCD)
void build_cell_tables(const PgPlan& P, const PlanLayout& A, size_t B, std::vector<uint32_t>& ct, std::vector<uint32_t>& cb, size_t& per)
{
    ct.assign((size_t)A.cells * 16, 0u);
    for (int l = 0; l < P.nlevels; l++) {
        const PgLevel& V = P.lvl[l];
        const int maxBorderX = V.w - PG_EDGE, maxBorderY = V.h - PG_EDGE;
        for (int i = 0; i < V.nRows; i++)
            for (int j = 0; j < V.nCols; j++) {
                const int cidx = i * V.nCols + j;
                uint32_t* r = &ct[((size_t)V.cellBase + cidx) * 16];
                const int iniY = PG_EDGE + i * V.hCell, iniX = PG_EDGE + j * V.wCell;      // :791-801
                const int W = std::min(iniX + V.wCell + 6, maxBorderX) - iniX;
                const int H = std::min(iniY + V.hCell + 6, maxBorderY) - iniY;
                // skipped cells (:794, :803) and windows cv::FAST finds nothing in (< 7 px)
                const bool skip = iniY >= maxBorderY - 3 || iniX >= maxBorderX - 6 || W < 7 || H < 7;
                const uint64_t off = (uint64_t)(A.pyrOff[l] * B) + (uint64_t)iniY * V.pitch + (uint64_t)(iniX - 1);
                r[0] = (uint32_t)l | ((uint32_t)(V.cellBase + cidx) << 4);
                r[1] = (uint32_t)iniX | ((uint32_t)iniY << 16);
                r[2] = (uint32_t)(skip ? 0 : W) | ((uint32_t)(skip ? 0 : H) << 8) | ((uint32_t)skip << 16) | ((uint32_t)V.cellCap << 17);
                r[3] = (uint32_t)V.pitch;
                r[4] = (uint32_t)off; r[5] = (uint32_t)(off >> 32);
                r[6] = (uint32_t)V.fstride;
                r[7] = (uint32_t)(V.cellCandOff + (int64_t)cidx * V.cellCap);
                // w8-w15: which lanes / result bits of the necessary test lie inside the interior, as LANE MASKS and bit
                // patterns (fast.hip, quick_pass_b: lane = quad (lane & 7) x row lr = 2 ((lane >> 3) & 3) + (lane >> 5), steps of 8
                // rows) -- a per-cell constant that used to cost every wave 17 vector instructions
                const int IW = W - 6, IH = H - 6;
                if (!skip && IW <= 32 && IH <= 40) {
                    const int qFull = IW >> 2, rem = IW & 3, base = IH >> 3, rr = IH & 7;
                    r[8] = ((1u << qFull) - 1u) * 0x01010101u;                     // lanes of whole quads (both 32-lane halves)
                    r[9] = qFull < 8 ? (1u << qFull) * 0x01010101u : 0u;           // lanes of the partial quad
                    r[10] = (1u << (8 * rem)) - 1u;                                // its pixels, one byte each
                    const int kLo = (rr + 1) >> 1, kHi = rr >> 1;                  // lanes whose row takes one step more than IH / 8
                    r[11] = kLo >= 4 ? 0xFFFFFFFFu : (1u << (8 * kLo)) - 1u;       //   lanes 0-31: lr = 2 (lane >> 3)
                    r[12] = (1u << (8 * kHi)) - 1u;                                //   lanes 32-63: lr = 2 ((lane >> 3) & 3) + 1
                    r[13] = ((1u << std::min(base, 4)) - 1u) * 0x11111111u;        // step bits every row has
                    r[14] = base < 4 ? 0x11111111u << base : 0u;                   // the step more
                    r[15] = base >= 5 ? 2u : (base == 4 ? 1u : 0u);                // fifth step: all rows / the rows of w11-w12 / none
                }
            }
    }
    // balanced dispatch order (fast.hip, k_fast_cells): XCD x takes cells [n_l x / 8, n_l (x + 1) / 8) of every level l
    std::vector<std::vector<int>> lists(8);
    for (int x = 0; x < 8; x++)
        for (int l = 0; l < P.nlevels; l++) {
            const PgLevel& V = P.lvl[l];
            const int n = V.nCols * V.nRows;
            for (int k = (int)((int64_t)n * x / 8); k < (int)((int64_t)n * (x + 1) / 8); k++) lists[x].push_back(V.cellBase + k);
        }
    per = 0;
    for (auto& v : lists) per = std::max(per, v.size());
    cb.assign(8 * per * 16, 0u);
    for (int x = 0; x < 8; x++)
        for (size_t k = 0; k < per; k++) {
            uint32_t* r = &cb[((size_t)x * per + k) * 16];
            if (k < lists[x].size()) memcpy(r, &ct[(size_t)lists[x][k] * 16], 64);
            else { r[0] = 0xFFFFFFF0u; r[2] = 1u << 16; }                                // padding: the wave returns at once
        }
}

// K3's coordinate tables for its pass kernel (quadtree.hip, k_qt_leaves: leaf column / row and candidate-order rank are separable
// in x and y), per level: [regionW] x entries, [regionH] y entries, [2^D + 1] first y of every leaf row; sets each level's qtTabOff
std::vector<uint2> build_qt_tables(PgPlan& P)
{
    std::vector<uint2> qt;
    for (int l = 0; l < P.nlevels; l++) {
        PgLevel& V = P.lvl[l];
        const int regionW = V.w - 2 * PG_EDGE, regionH = V.h - 2 * PG_EDGE, D = qt_pyr_depth(V.nIni);
        V.qtTabOff = (int32_t)qt.size();
        for (int x = 0; x < regionW; x++) {
            const uint2 e = qt_tab_entry(false, x, V.hX, V.nIni, regionH, D, V.wCell, V.hCell, V.nCols);
            qt.push_back(make_uint2(((e.x >> (2 * D)) << D) | qt_compact_bits(e.x & ((1u << (2 * D)) - 1)), e.y));
        }
        std::vector<int> rowY((size_t)(1 << D) + 1, regionH);
        for (int y = regionH - 1; y >= 0; y--) {
            const uint2 e = qt_tab_entry(true, y, V.hX, V.nIni, regionH, D, V.wCell, V.hCell, V.nCols);
            const uint32_t row = qt_compact_bits(e.x >> 1);
            for (uint32_t r = 0; r <= row; r++) rowY[r] = std::min(rowY[r], y);       // first y whose row is >= r
        }
        for (int y = 0; y < regionH; y++) {
            const uint2 e = qt_tab_entry(true, y, V.hX, V.nIni, regionH, D, V.wCell, V.hCell, V.nCols);
            qt.push_back(make_uint2(qt_compact_bits(e.x >> 1), e.y));
        }
        for (int r = 0; r <= (1 << D); r++) qt.push_back(make_uint2((uint32_t)rowY[r], 0u));
    }
    return qt;
}

}  // namespace

// Build (or reuse) the plan for w x h frames and a batch of `nframes`, on the context's device (which it makes current).
int make_plan(pgorb_ctx* c, int w, int h, int nframes)
{
    PG_HIP(c, hipSetDevice(c->prm.device));
    if (w > c->prm.max_width || h > c->prm.max_height)
        return fail(c, PGORB_E_LIMIT, "frame %dx%d exceeds context maximum %dx%d", w, h,
                    c->prm.max_width, c->prm.max_height);
    if (nframes > c->prm.max_batch)
        return fail(c, PGORB_E_LIMIT, "batch %d exceeds max_batch %d", nframes, c->prm.max_batch);
    if (c->planValid && c->planW == w && c->planH == h) return 0;

    const int L = c->prm.nlevels, B = c->prm.max_batch;
    LevelGeom g[PG_MAXL];
    int rc = level_geometry(c, w, h, g);
    if (rc) return fail(c, rc, "frame %dx%d too small: every pyramid level needs >= 62 px per side "
                               "and aspect >= 0.5", w, h);
    // the old plan dies here: a failure below (allocation, copy, limit) must not leave planValid set for
    // arenas that were already resized or a plan that is half written.  Work still in flight on any stream
    // (pgorb_stream_* batches, *_device calls on the caller's stream) reads the old tables and arenas: drain it
    // before they are overwritten.
    c->planValid = false;
    PG_HIP(c, hipDeviceSynchronize());
    PgPlan& P = c->plan;
    memset(&P, 0, sizeof(P));
    memset(&c->fuse, 0, sizeof(c->fuse));
    P.nlevels = L; P.iniTh = c->prm.ini_th_fast; P.minTh = c->prm.min_th_fast;
    P.tieMode = c->prm.blur_tie_mode;

    // --- host tables ---
    PlanLayout A;
    if ((rc = build_layout(c, g, P, A))) return rc;
    // resize tables, and the fused tables of the source level, of every level l >= 1: 16-aligned in one blob
    std::vector<uint8_t> tab;
    struct Fix { void* field; size_t off; };                         // the device-pointer field of P / c->fuse that takes tables.p + off
    std::vector<Fix> fix;
    auto put = [&](auto& field, const auto& v, bool used = true) {    // (a table the kernels cannot use keeps its place and a null pointer)
        const size_t off = align_up(tab.size(), 16), n = v.size() * sizeof(v[0]);
        tab.resize(off + n);
        memcpy(tab.data() + off, v.data(), n);
        if (used) fix.push_back({&field, off});
    };
    int pyrGpw = 2;                                                   // 4-row groups per wave of the LDS-staged resize
    if (const char* e = getenv("PGORB_PYR_TILE_ROWS")) { const int r = atoi(e); if (r == 16 || r == 32 || r == 64) pyrGpw = r / 16; }
    for (int l = 1; l < L; l++) {
        PgLevel& V = P.lvl[l];
        const ResizeTabs R = build_resize_level(g[l - 1], g[l], pyrGpw);
        put(V.xofs, R.xofs); put(V.xofs1, R.xofs1); put(V.xalpha, R.xalpha); put(V.yofs, R.yofs); put(V.ybeta, R.ybeta);
        put(V.qtab, R.qt, R.hasQ); put(V.qtab2, R.q2, R.hasQ2); put(V.yrel, R.yrel, R.hasY);
        put(V.rowgrp, R.rg); put(V.tilex, R.tilex);
        V.pyrCpr = R.cpr; V.pyrRows = R.prows; V.pyrGpw = pyrGpw;
        const FusedTabs F = build_fused_level(g[l - 1], g[l], R);
        if (F.nb > 0) {                                     // the fused tables belong to the SOURCE level l - 1
            PgFuseLevel& SV = c->fuse.lvl[l - 1];
            put(SV.bands, F.bands); put(SV.cols, F.cols);
            SV.nBands = F.nb; SV.spb = F.spb; SV.rows = F.rows;
        }
    }
    std::vector<uint32_t> ct, cb;
    size_t per = 0;
    build_cell_tables(P, A, B, ct, cb, per);
    const std::vector<uint2> qt = build_qt_tables(P);

    // --- arenas and uploads ---
    if ((rc = ensure(c, c->tables, tab.size() + 16))) return rc;
    if (!tab.empty()) PG_HIP(c, hipMemcpy(c->tables.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    if ((rc = ensure(c, c->pyr, A.pyrFrame * B))) return rc;
    if ((rc = ensure(c, c->cand, A.candFrame * 8 * B))) return rc;          // uint2 key records
    if ((rc = ensure(c, c->cellCand, A.cellCandFrame * 4 * B + 64))) return rc;      // (+64: K3's pass reads a cell's slots 16 bytes at a time)
    if ((rc = ensure(c, c->cellCount, (size_t)A.cells * 4 * B + 64))) return rc;
    if ((rc = ensure(c, c->sel, A.selFrame * 32 * B))) return rc;           // one 32-byte selection record per keypoint (quadtree.hip, PgSelRec)
    if ((rc = ensure(c, c->nodes, A.nodeFrame * 4 * B + 64))) return rc;
    if ((rc = ensure(c, c->counters, (size_t)B * PG_MAXL * 4 * 2 + 64))) return rc;
    // per-level counts: K3 writes the entries of the plan's levels in every batch, the others stay zero from here on (K4-6 sums all 16)
    PG_HIP(c, hipMemset(c->counters.p, 0, (size_t)B * PG_MAXL * 4 * 2 + 64));
    // + slack: a K2 wave loads its record BEFORE it knows whether the position exists (fast.hip), and the last workgroup's positions
    // run up to waves per workgroup x records per wave (4 x 64) past the table (round 6: 8 records of slack faulted under
    // "fast_cells_per_wave" = 64 when the table happened to end a mapping)
    const size_t cellTabSlack = (size_t)(4 * 64 + 8) * 64;
    if ((rc = ensure(c, c->cellTab, ct.size() * 4 + cellTabSlack))) return rc;
    PG_HIP(c, hipMemcpy(c->cellTab.p, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
    if ((rc = ensure(c, c->cellTabBal, cb.size() * 4 + cellTabSlack))) return rc;
    PG_HIP(c, hipMemcpy(c->cellTabBal.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice));
    if ((rc = ensure(c, c->qtTab, qt.size() * sizeof(uint2) + 64))) return rc;
    PG_HIP(c, hipMemcpy(c->qtTab.p, qt.data(), qt.size() * sizeof(uint2), hipMemcpyHostToDevice));
    if ((rc = ensure(c, c->qtLeaf, (size_t)B * L * PG_QT_LEAF_CAP * sizeof(uint2)))) return rc;
    // the status word heads the result block of the host-frame calls (pgorb_extract*: one download brings status, counts,
    // keypoints and descriptors); K1's first launch of a batch clears it
    const size_t ob = 64 + (((size_t)B * 4 + 63) & ~(size_t)63) + (((size_t)B * A.selTotal * sizeof(pgorb_keypoint) + 63) & ~(size_t)63) + (size_t)B * A.selTotal * 32 + 64;
    if ((rc = ensure(c, c->outBlk, ob))) return rc;
    PG_HIP(c, hipMemset(c->outBlk.p, 0, 64));
    // the memset runs on the null stream and may return before it has executed; the host-frame calls launch on a private
    // NON-BLOCKING stream (no implicit order with stream 0), so make it land before anything can write a status
    PG_HIP(c, hipStreamSynchronize(nullptr));

    // --- device pointers ---
    for (const Fix& f : fix) {
        const uint8_t* p = (const uint8_t*)c->tables.p + f.off;
        memcpy(f.field, &p, sizeof(p));
    }
    for (int l = 0; l < L; l++) P.lvl[l].img = (uint8_t*)c->pyr.p + A.pyrOff[l] * B;      // level-major: frames of a level adjacent
    P.cellCand = (uint32_t*)c->cellCand.p; P.cellCount = (int32_t*)c->cellCount.p;
    P.cellTab = (const uint32_t*)c->cellTab.p;
    P.cellTabBal = (const uint32_t*)c->cellTabBal.p;
    P.cellsPerXcdBal = (int)per;
    P.pyrBase = (const uint8_t*)c->pyr.p;
    P.qtTab = (const uint2*)c->qtTab.p; P.qtLeaf = (uint2*)c->qtLeaf.p;
    const char* wide = getenv("PGORB_QT_WIDE");
    P.qtWide = wide ? atoi(wide) != 0 : 1;
    P.cand = (uint32_t*)c->cand.p; P.sel = (uint32_t*)c->sel.p;
    P.nodeScratch = (int32_t*)c->nodes.p;
    P.candCount = (int32_t*)c->counters.p;
    P.kpCount = P.candCount + (size_t)B * PG_MAXL;
    P.status = (int32_t*)c->outBlk.p;
    c->planW = w; c->planH = h; c->planBatch = B; c->planValid = true;
    c->planEpoch++;                                            // (captured graphs hold the old plan by value)
    return 0;
}
