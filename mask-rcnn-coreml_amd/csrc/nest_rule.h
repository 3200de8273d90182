// nest_rule.h — the rule of mrcnn_polygons_nest (polygon rings nested into outlines and their holes), written once for the device and
// the host: a ring's doubled area, its probe, the crossing test of one edge, and the two orders that pick a parent.  The host definition
// (nest_host.cpp) loops over rings and edges one by one; the kernels (kernels_nest.hip) give a workgroup a ring and its waves the
// candidates.  Integers only: no division, no floating point.
//
// The rule.  Rings in the tracer's layout, closed, every coordinate in 0..32767 (NEST_COORD_MAX); the rings of one RLE are nested among
// themselves and never with those of another.
//   area2(r)        twice the signed shoelace area, sum(x_i*y_{i+1} - x_{i+1}*y_i) round the ring, from xy itself (under 2^62 in size).
//   probe(r)        the point (X0 + 1/2, Y0 + 1/2), (X0, Y0) the ring's FIRST vertex.  A ring without vertices has no probe and no parent.
//                   For a traced ring it is the centre of a pixel the ring encloses, a set pixel for an outline and an unset one for a
//                   hole: the ring starts at its smallest vertex (x, then y) and nothing of it lies left of that vertex, so the unit edge
//                   (X0, Y0) - (X0, Y0 + 1) is the only piece of the ring that a ray from the probe towards -x meets.
//   contains(q, r)  the ray from probe(r) towards -x crosses an odd number of q's edges, the closing edge included.  An edge a -> b
//                   crosses iff (ay <= Y0) != (by <= Y0) and its point on the line y = Y0 + 1/2 lies at x < X0 + 1/2: with all lengths
//                   doubled that is the sign of the cross product (b - a) x (P - a), P = (2*X0 + 1, 2*Y0 + 1), corrected by the sign
//                   of by - ay (64 bits; a product of 0 is a probe ON the edge, which is not left of it: no crossing).  No vertex lies on
//                   the ray's line — a doubled vertex is even, P is odd —, so no crossing is counted twice.  For an axis-parallel ring
//                   this counts the vertical edges with x <= X0 whose y-span holds Y0.  A ring of fewer than 3 vertices contains nothing.
//   parent(r)       among the rings q != r of r's RLE with contains(q, r) that OUTRANK r — |area2(q)| > |area2(r)|, or equal and
//                   q < r — the one of smallest |area2|, the smallest index on a tie; -1 if there is none.  Outranking is a strict total
//                   order, so the parents form a forest on any input.  On traced rings it is the innermost ring round r.
//   depth(r)        the number of ancestors.  On traced rings even = outline (area > 0), odd = hole; a hole's parent is the outline of the
//                   4-connected component round it, an outline's parent the hole it is an island of.
//   polygons        a ring of even depth is a SHELL, its children (odd depth) are its holes.  The polygons of an RLE are ordered by their
//                   shell's ring index; inside a polygon the shell comes first, then its holes by ring index.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MRCNN_NR_HD __host__ __device__ __forceinline__
#else
#define MRCNN_NR_HD inline
#endif

namespace mrcnn {

constexpr int NEST_COORD_MAX = 32767;

// one term of area2: the edge a -> b
MRCNN_NR_HD int64_t nest_area_term(int ax, int ay, int bx, int by) { return (int64_t)ax * by - (int64_t)bx * ay; }

MRCNN_NR_HD uint64_t nest_abs(int64_t area2) { return area2 < 0 ? (uint64_t)(-area2) : (uint64_t)area2; }

// does the edge a -> b cross the ray from (X0 + 1/2, Y0 + 1/2) towards -x
MRCNN_NR_HD bool nest_crosses(int ax, int ay, int bx, int by, int X0, int Y0)
{
    if ((ay <= Y0) == (by <= Y0)) return false;
    const int64_t dy = by - ay;                                                              // not 0
    // (b - a) x (P - a) with P - a in doubled lengths, (2*X0 + 1 - 2*ax, 2*Y0 + 1 - 2*ay), and b - a as it is: half the doubled cross product,
    // the same sign.  Each factor is under 2^15 and 2^16 in size, each product under 2^31, the difference under 2^32.
    const int64_t cross = (int64_t)(bx - ax) * (2 * Y0 + 1 - 2 * ay) - dy * (2 * X0 + 1 - 2 * ax);
    return dy > 0 ? cross < 0 : cross > 0;                                                   // the edge's point on the line lies left of the probe
}

// ring q (|area2| = aq) may be an ancestor of ring r (|area2| = ar)
MRCNN_NR_HD bool nest_outranks(uint64_t aq, int64_t q, uint64_t ar, int64_t r) { return aq > ar || (aq == ar && q < r); }

// of two rings that contain a probe, q is the closer one
MRCNN_NR_HD bool nest_closer(uint64_t aq, int64_t q, uint64_t ab, int64_t b) { return aq < ab || (aq == ab && q < b); }

}  // namespace mrcnn
