// poly_device.h — COCO's rleFrPoly in closed form: the arithmetic of polygon_toggles (api_coco.hip) per edge and per pixel column,
// without the walk over the fine grid.  Host and device compile the same text; the device side is built with -ffp-contract=off
// (kernels_coco.hip), so every product and sum below is rounded once, as on the x86 host, and the divisions are IEEE fp64 divisions.
//
// polygon_toggles walks every point of every edge on a grid five times finer than the pixels: point t of an edge is
//     x-major (dx >= dy):  u = xs + t,  v = (int)(ys + s*t + .5)        y-major:  v = ys + t,  u = (int)(xs + s*t + .5)
// for t = 0 .. span (the order of the walk does not matter: what counts are the pairs (t, t+1)), and a pair of neighbouring points is a
// run boundary when u differs and the lower u is 5k + 2 for a pixel column k in 0 .. w-1 ((u + .5) / 5 - .5 = k exactly, and for no
// other u an integer).  Pairs across the junction of two edges never count: both points stand for the same vertex, and where their u
// differ (the truncation of a negative x) the lower one is negative.
//   x-major: u moves by exactly one per step, so column k is crossed once, between t = 5k + 2 - xs and t + 1, when both lie on the edge.
//   y-major: |s| < 1, so u(t) is monotone and moves by at most one per step: column k is crossed once when 5k + 2 and 5k + 3 both lie
//   between u(0) and u(span); the step is found by bisection on the computed u itself.
// So an edge has `cnt` boundaries, those of the columns klo .. klo + cnt - 1, and each is evaluated on its own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_HD __host__ __device__ __forceinline__
#else
#define MRCNN_HD inline
#endif

namespace mrcnn {

struct PolyEdge {
    long xs, ys, span;      // the start after the flip (the end with the lower major coordinate)
    double s;               // minor step per major step
    int xmajor, rising;     // rising: u grows with t (y-major only)
    int klo, cnt;           // the pixel columns whose centre this edge crosses: klo .. klo + cnt - 1
};

MRCNN_HD long poly_quant(double c) { return (long)(int)(5.0 * c + .5); }
MRCNN_HD long poly_floordiv5(long a) { return a >= 0 ? a / 5 : -((-a + 4) / 5); }
// the minor coordinate of point t: (int)(start + s*t + .5), truncating like the host's conversion
MRCNN_HD long poly_minor(long start, double s, long t) { return (long)(int)((double)start + s * (double)t + .5); }

// the edge from fine point (x0, y0) to (x1, y1) on a plane `w` pixels wide
MRCNN_HD PolyEdge poly_edge(long x0, long y0, long x1, long y1, int w)
{
    PolyEdge e;
    long xs = x0, xe = x1, ys = y0, ye = y1;
    const long dx = xe > xs ? xe - xs : xs - xe, dy = ys > ye ? ys - ye : ye - ys;
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { long t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    e.xmajor = dx >= dy;
    e.span = e.xmajor ? dx : dy;
    e.s = e.span == 0 ? 0.0 : (e.xmajor ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy);
    e.xs = xs; e.ys = ys;
    long lo, hi;
    if (e.xmajor) { lo = xs; hi = xe; e.rising = 1; }
    else {
        const long ua = poly_minor(xs, e.s, 0), ub = poly_minor(xs, e.s, e.span);
        e.rising = ub > ua;
        lo = e.rising ? ua : ub; hi = e.rising ? ub : ua;
    }
    // columns k with lo <= 5k + 2 and 5k + 3 <= hi, inside the plane
    long klo = -poly_floordiv5(-(lo - 2)), khi = poly_floordiv5(hi - 3);
    if (klo < 0) klo = 0;
    if (khi > (long)w - 1) khi = (long)w - 1;
    e.klo = (int)klo;
    e.cnt = khi >= klo ? (int)(khi - klo + 1) : 0;
    return e;
}

// the position (column-major, 0 .. h*w) where the stream toggles because edge `e` crosses the centre of pixel column k
MRCNN_HD uint32_t poly_toggle(const PolyEdge& e, int k, int h)
{
    long v;
    if (e.xmajor) {
        const long t = 5L * k + 2 - e.xs;
        const long v0 = poly_minor(e.ys, e.s, t), v1 = poly_minor(e.ys, e.s, t + 1);
        v = v0 < v1 ? v0 : v1;
    } else {
        // the first t1 in 1 .. span behind the crossing: u(t1) >= 5k + 3 (rising) or u(t1) <= 5k + 2 (falling); the pair is (t1 - 1, t1)
        const long bar = 5L * k + (e.rising ? 3 : 2);
        long a = 1, b = e.span;
        while (a < b) {
            const long mid = (a + b) >> 1;
            const long u = poly_minor(e.xs, e.s, mid);
            if (e.rising ? u >= bar : u <= bar) b = mid; else a = mid + 1;
        }
        v = e.ys + a - 1;
    }
    double yd = ((double)v + .5) / 5.0 - .5;
    if (yd < 0) yd = 0; else if (yd > (double)h) yd = (double)h;
    yd = __builtin_ceil(yd);
    return (uint32_t)((long)k * h + (long)yd);
}

}  // namespace mrcnn
