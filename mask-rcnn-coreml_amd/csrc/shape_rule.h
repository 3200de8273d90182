// shape_rule.h — the rules of mrcnn_rle_measure and mrcnn_rle_convex_hull, written once for the device and the host (include/maskrcnn_hip.h
// states them in full): the closed forms of a column piece's and a block of full columns' moments, the walking order of the hull's
// candidates, the chain rule that picks and keeps a hull vertex, and the oriented box of a hull edge with the comparison of two boxes.
// Integers only.  The host definition (rle_shape_host.cpp) sums pixel by pixel and runs Andrew's monotone chain; the kernels
// (kernels_rle_shape.hip) use the closed forms and QuickHull level by level.  The hull is unique, so both give the same ring.
//
// Ranges.  Sides are at most 32767, pixel indices at most 32766, corners at most 32767.
//   moments   S1 <= 32767^2 < 2^30; Sx, Sy < 32767^3 / 2 < 2^44; Sxx, Syy, Sxy < 32767^4 / 3 < 2^59 (< 2^60): every word fits int64, and so
//             does every partial sum below.  perimeter <= 4 * S1 < 2^32.
//   chain     c(p) is the difference of two products of corner differences: |c| <= 2 * 32767^2 < 2^31, so a positive c is the 32-bit
//             distance of simplify_rule.h's key, and the key with the position is the same 64-bit maximum.
//   box       |d|, |c| <= 2 * 32767^2 < 2^31, D, C < 2^32; D * C = L2 * (the rectangle's area) <= 2^31 * 2^31: 64 bits unsigned; times the
//             other edge's L2 < 2^31: 94 bits at most, compared with simplify_rule.h's 128-bit product.
#pragma once
#include <stdint.h>

#include "simplify_rule.h"

namespace mrcnn {

constexpr int SHAPE_MEASURE_WORDS = 7;     // S1, Sx, Sy, Sxx, Sxy, Syy, perimeter
constexpr int SHAPE_OBB_WORDS = 8;         // e, dx, dy, dmin, dmax, cmin, cmax, 0

// ---- moments ------------------------------------------------------------------------------------------------------------------------
struct ShapeMoments { int64_t s1, sx, sy, sxx, sxy, syy; };

// the sums of t and of t^2 over 0 <= t < n
MRCNN_SP_HD int64_t shape_sum1(int64_t n) { return n * (n - 1) / 2; }
MRCNN_SP_HD int64_t shape_sum2(int64_t n) { return (n - 1) * n * (2 * n - 1) / 6; }

// rows [a, b) of pixel column x
MRCNN_SP_HD void shape_add_piece(ShapeMoments& m, int64_t x, int64_t a, int64_t b)
{
    const int64_t cnt = b - a, y1 = shape_sum1(b) - shape_sum1(a), y2 = shape_sum2(b) - shape_sum2(a);
    m.s1 += cnt; m.sx += x * cnt; m.sy += y1;
    m.sxx += x * x * cnt; m.sxy += x * y1; m.syy += y2;
}

// the full pixel columns [xa, xb) of a plane of h rows, whatever their number
MRCNN_SP_HD void shape_add_columns(ShapeMoments& m, int64_t xa, int64_t xb, int64_t h)
{
    const int64_t nc = xb - xa, x1 = shape_sum1(xb) - shape_sum1(xa), x2 = shape_sum2(xb) - shape_sum2(xa);
    const int64_t y1 = shape_sum1(h), y2 = shape_sum2(h);
    m.s1 += nc * h; m.sx += x1 * h; m.sy += nc * y1;
    m.sxx += x2 * h; m.sxy += x1 * y1; m.syy += nc * y2;
}

// a run of n > 0 set pixels from column-major position s (x * h + y) of a plane of h rows: a head piece, full columns, a tail piece
MRCNN_SP_HD void shape_add_run(ShapeMoments& m, uint32_t s, uint32_t n, int h)
{
    const uint32_t e = s + n, H = (uint32_t)h;
    const int64_t x0 = s / H, y0 = s - (uint32_t)x0 * H, x1 = (e - 1) / H, y1 = e - (uint32_t)x1 * H;     // y1 in 1..h
    if (x0 == x1) { shape_add_piece(m, x0, y0, y1); return; }
    shape_add_piece(m, x0, y0, h);
    if (x1 > x0 + 1) shape_add_columns(m, x0 + 1, x1, h);
    shape_add_piece(m, x1, 0, y1);
}

// ---- the hull's candidates ------------------------------------------------------------------------------------------------------------
// A plane of w pixel columns has the vertex columns X = 0 .. w.  Pixel column x with set pixels has the first set row t(x) and one past
// the last, b(x).  Vertex column X has candidates when pixel column X - 1 or X has set pixels: T(X) the smaller t and B(X) the larger b
// of those.  The candidates in walking order (clockwise on screen, y down), 2 * (w + 1) positions:
//   position X, 0 <= X <= w              the top chain      (X, T(X)), rising X
//   position 2 * w + 1 - X, 0 <= X <= w  the bottom chain   (X, B(X)), falling X
// The first and the last candidate of each chain are hull vertices (the ring starts at the first of the top chain: the smallest vertex by
// x then y); between them QuickHull, or any other method, keeps the candidates strictly left of every chord.
MRCNN_SP_HD int shape_positions(int w) { return 2 * (w + 1); }
MRCNN_SP_HD int shape_position_x(int pos, int w) { return pos <= w ? pos : 2 * w + 1 - pos; }
MRCNN_SP_HD bool shape_position_top(int pos, int w) { return pos <= w; }

// c(p) of the directed chord a -> b: positive when p lies left of it, which on screen is outside the chord of a clockwise ring
MRCNN_SP_HD int64_t shape_cross(int ax, int ay, int bx, int by, int px, int py)
{
    return (int64_t)(by - ay) * (px - ax) - (int64_t)(bx - ax) * (py - ay);
}
// The choice among the candidates between a and b as simplify_rule.h's maximum: the largest c, then the smallest position.  A candidate
// on the chord or right of it offers distance 0, and a winner of distance 0 is not kept: the strict test drops collinear points.
MRCNN_SP_HD uint64_t shape_key(int64_t c, int position) { return simp_key(c > 0 ? (uint32_t)c : 0u, position); }
MRCNN_SP_HD bool shape_keeps(uint64_t key) { return simp_key_distance(key) > 0; }

// ---- the oriented box ---------------------------------------------------------------------------------------------------------------
// the box of one hull edge: its vector, the extremes of d = dx*X + dy*Y and c = dx*Y - dy*X over the hull's vertices
struct ShapeBox { int64_t dx, dy, dmin, dmax, cmin, cmax; };

// X(i), Y(i): vertex i of a hull of m vertices; the edge e runs from vertex e to vertex e + 1 (cyclic)
template <class GetX, class GetY>
MRCNN_SP_HD ShapeBox shape_edge_box(int m, int e, GetX X, GetY Y)
{
    const int f = e + 1 < m ? e + 1 : 0;
    ShapeBox b;
    b.dx = (int64_t)X(f) - X(e); b.dy = (int64_t)Y(f) - Y(e);
    b.dmin = b.cmin = INT64_MAX; b.dmax = b.cmax = INT64_MIN;
    for (int i = 0; i < m; ++i) {
        const int64_t x = X(i), y = Y(i), d = b.dx * x + b.dy * y, c = b.dx * y - b.dy * x;
        b.dmin = d < b.dmin ? d : b.dmin; b.dmax = d > b.dmax ? d : b.dmax;
        b.cmin = c < b.cmin ? c : b.cmin; b.cmax = c > b.cmax ? c : b.cmax;
    }
    return b;
}

// what two boxes are compared by: D * C and L2; the rectangle's area is their quotient
struct ShapeScore { uint64_t dc, l2; };
MRCNN_SP_HD ShapeScore shape_score(const ShapeBox& b)
{
    return ShapeScore{(uint64_t)(b.dmax - b.dmin) * (uint64_t)(b.cmax - b.cmin), (uint64_t)(b.dx * b.dx + b.dy * b.dy)};
}
// is edge i's box chosen before edge j's: the smaller area, exactly; the smaller edge on a tie
MRCNN_SP_HD bool shape_box_before(const ShapeScore& a, int i, const ShapeScore& b, int j)
{
    const SimpU128 l = simp_mul64(a.dc, b.l2), r = simp_mul64(b.dc, a.l2);
    if (l.hi != r.hi || l.lo != r.lo) return simp_greater(r, l);
    return i < j;
}

}  // namespace mrcnn
