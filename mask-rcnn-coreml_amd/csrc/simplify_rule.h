// simplify_rule.h — the rule of mrcnn_polygons_simplify (Douglas-Peucker on closed integer rings), written once for the device and the
// host: the tolerance as one integer, the two distances, the exact threshold test, the key that picks a chain's vertex and the ring's
// second anchor.  The host definition (simplify_host.cpp) recurses with an explicit stack; the kernels (kernels_simplify.hip) run the
// same chains level by level.  Integers only: nothing after simp_tolerance touches floating point.
//
// The rule.  A closed ring of m vertices v_0 .. v_{m-1}, every coordinate in 0..32767 (SIMP_COORD_MAX):
//   m <= 2     the ring is copied as it is.
//   anchors    v_0, the ring's start, and v_f, the vertex of largest squared Euclidean distance from v_0, the smallest index on a tie
//              (f = 0 when every vertex equals v_0).  Both are kept.
//   chains     the two open chains v_0 .. v_f and v_f .. v_m (v_m is v_0 again) are simplified independently.
//   a chain    with end vertices a and b and at least one vertex strictly between them: every such vertex p has a distance
//                c(p) = |(b - a) x (p - a)|   when a and b differ in a coordinate (at most 2 * 32767^2: 32 bits),
//                c(p) = |p - a|^2             when a and b have equal coordinates (a ring may pass twice through a vertex).
//              The chosen vertex has the largest c, the smallest position along the chain on a tie.  It is KEPT iff
//                c^2 * 65536 > E * |b - a|^2  (a != b; exact, 128 bits)        c * 65536 > E  (a = b)
//              and then the two chains a .. p and p .. b are handled in the same way; otherwise every vertex strictly between a and b is
//              dropped.  E = floor(tolerance^2 * 65536): a vertex is kept iff its distance from the chord exceeds the tolerance, to 1/256 px.
// What follows.  The output ring is a subsequence of the input ring and starts at the same vertex; rings stay in their order, one for
// one.  Tolerance 0 (E = 0) keeps every vertex that is not on its chord: a traced ring, whose horizontal and vertical pieces alternate,
// has none and comes back unchanged.  The kept sets are nested: a larger tolerance keeps a subset.  A ring may come out with 2 vertices
// (1 if all its vertices are equal).  Rings may touch or cross one another afterwards: topology is not preserved.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MRCNN_SP_HD __host__ __device__ __forceinline__
#else
#define MRCNN_SP_HD inline
#endif

namespace mrcnn {

constexpr int SIMP_COORD_MAX = 32767;
constexpr double SIMP_TOLERANCE_MAX = 65535.0;

// The tolerance as the rule's integer, once, on the host.  tol is finite, 0 <= tol <= SIMP_TOLERANCE_MAX: E < 2^48.
inline uint64_t simp_tolerance(double tol) { return (uint64_t)(tol * tol * 65536.0); }      // (two roundings, then exact: the product is not negative)

// an unsigned 128-bit number and the product of two 64-bit ones from 32-bit partial products
struct SimpU128 { uint64_t hi, lo; };

MRCNN_SP_HD SimpU128 simp_mul64(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);            // < 3 * 2^32
    SimpU128 r;
    r.lo = (p00 & 0xffffffffu) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}
MRCNN_SP_HD bool simp_greater(const SimpU128& a, const SimpU128& b) { return a.hi != b.hi ? a.hi > b.hi : a.lo > b.lo; }

MRCNN_SP_HD uint32_t simp_dist2(int ax, int ay, int bx, int by)                              // |b - a|^2 <= 2 * 32767^2 < 2^31
{
    const int64_t dx = bx - ax, dy = by - ay;
    return (uint32_t)(dx * dx + dy * dy);
}

// c(p) of the chain a .. b
MRCNN_SP_HD uint32_t simp_distance(int ax, int ay, int bx, int by, int px, int py)
{
    if (ax == bx && ay == by) return simp_dist2(ax, ay, px, py);
    const int64_t cross = (int64_t)(bx - ax) * (py - ay) - (int64_t)(by - ay) * (px - ax);   // |.| <= 2 * 32767^2
    return (uint32_t)(cross < 0 ? -cross : cross);
}

// is the chosen vertex of the chain a .. b, at distance c, kept
MRCNN_SP_HD bool simp_keeps(uint32_t c, uint64_t E, int ax, int ay, int bx, int by)
{
    if (ax == bx && ay == by) return ((uint64_t)c << 16) > E;                                // c < 2^31
    const uint64_t c2 = (uint64_t)c * c;                                                     // < 2^62
    const SimpU128 left{c2 >> 48, c2 << 16};
    return simp_greater(left, simp_mul64(E, simp_dist2(ax, ay, bx, by)));
}

// The choice as one maximum: the largest distance, then the smallest position (a ring has fewer than 2^31 vertices).  Never 0.
MRCNN_SP_HD uint64_t simp_key(uint32_t c, int position) { return ((uint64_t)c << 32) | (uint32_t)~(uint32_t)position; }
MRCNN_SP_HD uint32_t simp_key_distance(uint64_t key) { return (uint32_t)(key >> 32); }
MRCNN_SP_HD int simp_key_position(uint64_t key) { return (int)~(uint32_t)key; }

}  // namespace mrcnn
