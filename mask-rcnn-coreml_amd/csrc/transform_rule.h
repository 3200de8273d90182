// transform_rule.h — moving a run-length mask to another pixel grid, the rule written once for the device and the host
// (include/maskrcnn_hip.h states it in full).  A record [flags, ax, bx, dx, ay, by, dy, 0] sends the output pixel (X, Y) to the source pixel
//   u = floor((ax*X + bx) / dx), v = floor((ay*Y + by) / dy), (sx, sy) = (u, v), or (v, u) with MRCNN_XF_TRANSPOSE,
// and the output pixel is the source's when (sx, sy) lies inside the source plane, else 0.  The host definition
// (rle_transform_host.cpp) evaluates only this forward map, pixel by pixel on a decoded plane.  The kernel (kernels_rle_transform.hip)
// also needs the INVERSE — the range of X whose u falls into a range of source indices — which is here in closed form.  Floor
// division everywhere: a window that reaches outside the plane and every flip give negative numerators.
#pragma once
#include <stdint.h>

#include "morph_rule.h"

#ifdef __HIPCC__
#define MRCNN_XF_HD __host__ __device__ __forceinline__
#else
#define MRCNN_XF_HD inline
#endif

namespace mrcnn {

constexpr long long XF_MAX_A = 2147483647LL;                 // |ax|, |ay| and dx, dy lie in 1..2^31-1, |bx|, |by| <= 2^46:
constexpr long long XF_MAX_B = 1LL << 46;                    // with indices below 2^15 every product and sum stays inside int64

// one axis of a record: index i of the output goes to floor((a*i + b) / d) of the source
struct XfAxis { long long a, b, d; };
// a record as the kernels take it
struct XfMap { XfAxis x, y; int transpose, pad; };

// floor(n / d) and ceil(n / d) for d > 0 and any n (C++'s own division truncates towards zero)
MRCNN_XF_HD long long xf_floor_div(long long n, long long d) { const long long q = n / d; return (n % d != 0 && n < 0) ? q - 1 : q; }
MRCNN_XF_HD long long xf_ceil_div(long long n, long long d) { const long long q = n / d; return (n % d != 0 && n > 0) ? q + 1 : q; }

// the forward map of one axis
MRCNN_XF_HD long long xf_source(const XfAxis& m, long long i) { return xf_floor_div(m.a * i + m.b, m.d); }

// The inverse of one axis: [*lo, *hi) is the range of every integer i with lo_src <= xf_source(m, i) < hi_src (lo_src <= hi_src, both
// within +-2^15; the range is not clipped and is empty as lo >= hi).
//   a > 0:  a*i + b >= lo_src*d  <=>  i >= ceil((lo_src*d - b) / a),   and the same bound with hi_src ends the range
//   a < 0:  b - |a|*i >= lo_src*d  <=>  i <= floor((b - lo_src*d) / |a|);   b - |a|*i < hi_src*d  <=>  i > floor((b - hi_src*d) / |a|)
MRCNN_XF_HD void xf_preimage(const XfAxis& m, long long lo_src, long long hi_src, long long* lo, long long* hi)
{
    if (m.a > 0) {
        *lo = xf_ceil_div(lo_src * m.d - m.b, m.a);
        *hi = xf_ceil_div(hi_src * m.d - m.b, m.a);
    } else {
        *lo = xf_floor_div(m.b - hi_src * m.d, -m.a) + 1;
        *hi = xf_floor_div(m.b - lo_src * m.d, -m.a) + 1;
    }
}

// the same, clipped to the indices [c0, c1) of an output axis
MRCNN_XF_HD void xf_preimage_in(const XfAxis& m, long long lo_src, long long hi_src, int c0, int c1, int* lo, int* hi)
{
    long long l, h;
    xf_preimage(m, lo_src, hi_src, &l, &h);
    *lo = (int)(l < c0 ? c0 : (l > c1 ? c1 : l));
    *hi = (int)(h < c0 ? c0 : (h > c1 ? c1 : h));
}

// whether the eight words of a record are a record: flags 0 or MRCNN_XF_TRANSPOSE, the coefficients within their limits, word 7 zero
MRCNN_XF_HD bool xf_axis_known(long long a, long long b, long long d)
{
    return d >= 1 && d <= XF_MAX_A && a != 0 && a >= -XF_MAX_A && a <= XF_MAX_A && b >= -XF_MAX_B && b <= XF_MAX_B;
}

MRCNN_XF_HD XfMap xf_map(const int64_t* r)
{
    XfMap m;
    m.x = XfAxis{(long long)r[1], (long long)r[2], (long long)r[3]};
    m.y = XfAxis{(long long)r[4], (long long)r[5], (long long)r[6]};
    m.transpose = (int)(r[0] & MRCNN_XF_TRANSPOSE); m.pad = 0;
    return m;
}

// The box of the out_h x out_w output plane outside which the result is 0, from the tight box of the source's set pixels: the preimage
// of the box's columns and rows, each along the output axis that reads them (a transposed record reads source rows along X).  An
// empty tight box, or a preimage that misses the output plane, is the empty box (0, 0, 0, 0).
MRCNN_XF_HD MorphBox xf_work_box(const XfMap& m, const MorphBox& t, int out_h, int out_w)
{
    const MorphBox none{0, 0, 0, 0};
    if (t.y2 <= t.y1 || t.x2 <= t.x1) return none;
    MorphBox b;
    xf_preimage_in(m.x, m.transpose ? t.y1 : t.x1, m.transpose ? t.y2 : t.x2, 0, out_w, &b.x1, &b.x2);
    xf_preimage_in(m.y, m.transpose ? t.x1 : t.y1, m.transpose ? t.x2 : t.y2, 0, out_h, &b.y1, &b.y2);
    return (b.x1 < b.x2 && b.y1 < b.y2) ? b : none;
}

}  // namespace mrcnn
