// polygon_rule.h — the boundary rule of mrcnn_rle_to_polygons, written once for the device and the host: the four headings, which
// directed edges leave and reach a vertex, the turn the walk takes there, what makes a vertex a corner of a ring, and the two orders
// of corners (by column: the canonical start and the order of the rings; by row: the horizontal partner).  The host definition
// (polygons_host.cpp) walks unit edges with poly_out_edge / poly_turn; the kernels (kernels_polygons.hip) only ever look at corners,
// which poly_corners lists from the same two functions.  Integers only.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MRCNN_PG_HD __host__ __device__ __forceinline__
#else
#define MRCNN_PG_HD inline
#endif

namespace mrcnn {

// Headings, x right and y down as on screen.  The set pixel lies on the right of an edge, so an outline runs clockwise on screen and a
// right turn is the next heading: +x -> +y -> -x -> -y.
enum { POLY_PX = 0, POLY_PY = 1, POLY_MX = 2, POLY_MY = 3 };
MRCNN_PG_HD int poly_dx(int d) { return d == POLY_PX ? 1 : (d == POLY_MX ? -1 : 0); }
MRCNN_PG_HD int poly_dy(int d) { return d == POLY_PY ? 1 : (d == POLY_MY ? -1 : 0); }
MRCNN_PG_HD bool poly_vertical(int d) { return (d & 1) != 0; }

// The pixels round vertex (X, Y): tl = (X-1, Y-1), tr = (X, Y-1), bl = (X-1, Y), br = (X, Y), each 0 or 1 (0 outside the plane).
struct PolyNbhd { int tl, tr, bl, br; };

// the unit edge that LEAVES the vertex with heading d is a boundary edge: the pixel on its right is set, the one on its left is not
MRCNN_PG_HD bool poly_out_edge(int d, const PolyNbhd& n)
{
    switch (d) {
    case POLY_PX: return n.br && !n.tr;     // top edge of br
    case POLY_PY: return n.bl && !n.br;     // right edge of bl
    case POLY_MX: return n.tl && !n.bl;     // bottom edge of tl
    default:      return n.tr && !n.tl;     // left edge of tr
    }
}

// the unit edge that REACHES the vertex with heading e is a boundary edge
MRCNN_PG_HD bool poly_in_edge(int e, const PolyNbhd& n)
{
    switch (e) {
    case POLY_PX: return n.bl && !n.tl;     // top edge of bl
    case POLY_PY: return n.tl && !n.tr;     // right edge of tl
    case POLY_MX: return n.tr && !n.br;     // bottom edge of tr
    default:      return n.br && !n.bl;     // left edge of br
    }
}

// The turn rule: a walk that reaches the vertex with heading e leaves it by the first boundary edge among right turn, straight on, left
// turn.  Where two set pixels touch only diagonally all four edges are there and the walk turns right: it stays with its own pixel.
MRCNN_PG_HD int poly_turn(int e, const PolyNbhd& n)
{
    const int right = (e + 1) & 3, left = (e + 3) & 3;
    return poly_out_edge(right, n) ? right : (poly_out_edge(e, n) ? e : left);
}

// A corner of a ring: a vertex the walk reaches with heading `in` and leaves with another heading `out`; one of the two is vertical.
//   up    its vertical piece lies above the vertex (else below): in a vertex column sorted by (Y, !up) the corners 2j and 2j+1 are the
//         two ends of one vertical piece
//   left  its horizontal piece lies left of the vertex: in a vertex row sorted by (X, !left) likewise for the horizontal pieces
struct PolyCorner { int in, out; bool up, left; };

MRCNN_PG_HD PolyCorner poly_corner(int in, int out)
{
    PolyCorner c;
    c.in = in; c.out = out;
    c.up = in == POLY_PY || out == POLY_MY;
    c.left = in == POLY_PX || out == POLY_MX;
    return c;
}

// the corners at a vertex, the one with the upper vertical piece first: none, one, or two at a diagonal contact
MRCNN_PG_HD int poly_corners(const PolyNbhd& n, PolyCorner out[2])
{
    int m = 0;
    for (int e = 0; e < 4; ++e) {
        if (!poly_in_edge(e, n)) continue;
        const int d = poly_turn(e, n);
        if (d != e && m < 2) out[m++] = poly_corner(e, d);
    }
    if (m == 2 && !out[0].up) { const PolyCorner t = out[0]; out[0] = out[1]; out[1] = t; }
    return m;
}

// The order of vertices: x, then y.  A ring starts at its smallest vertex and the rings of a plane are listed by their starts.
MRCNN_PG_HD bool poly_vertex_less(int xa, int ya, int xb, int yb) { return xa != xb ? xa < xb : ya < yb; }

// A corner as the kernels keep it, 32 bits: bit 31 = it leaves by its vertical piece, bits 0..30 = its place in the row order
// (Y, X, !left): Y in bits 16..30, X in bits 1..15 (a side is at most 32767, so 0 <= X, Y <= 32767 take 15 bits each).
MRCNN_PG_HD uint32_t poly_pack(int x, int y, const PolyCorner& c)
{
    return ((uint32_t)poly_vertical(c.out) << 31) | ((uint32_t)y << 16) | ((uint32_t)x << 1) | (c.left ? 0u : 1u);
}
MRCNN_PG_HD int poly_packed_x(uint32_t p) { return (int)((p >> 1) & 0x7fffu); }
MRCNN_PG_HD int poly_packed_y(uint32_t p) { return (int)((p >> 16) & 0x7fffu); }
MRCNN_PG_HD bool poly_packed_leaves_vertically(uint32_t p) { return (p >> 31) != 0; }
MRCNN_PG_HD uint32_t poly_packed_row_key(uint32_t p) { return p & 0x7fffffffu; }

}  // namespace mrcnn
