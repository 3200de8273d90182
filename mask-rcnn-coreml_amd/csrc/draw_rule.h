// draw_rule.h — the drawing rule, written once for the device and the host: the stroke of a box, the palette, a pixel's code and the
// output byte, which the 28×28 kernels (kernels_render.hip), the RLE drawing kernels (kernels_rle_draw.hip) and their host definition
// (rle_draw_host.cpp) all call; and the two decisions about a detection row that the last two must take alike: its pixel box in its
// image's own frame and whether it is drawn.  The products are a float times an int below 2^15: exact in double, so the one rounding
// is rint's (half to even) on the device and on the host.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define MRCNN_RD_HD __host__ __device__ __forceinline__
#else
#define MRCNN_RD_HD inline
#endif

namespace mrcnn {

struct RleDrawBox { int y1, x1, y2, x2; };       // y2, x2 exclusive

// a user's own row may hold anything: a NaN is 0 and the value is held to +-2^20 (far outside any image), so the conversion is defined
MRCNN_RD_HD int rle_draw_round(double v)
{
    if (!(v == v)) v = 0.0;
    v = v < -1048576.0 ? -1048576.0 : (v > 1048576.0 ? 1048576.0 : v);
    return (int)rint(v);
}

// row = (y1, x1, y2, x2, class, score), normalised to the h x w image: round-half-even of y * (h - 1), + 1 on the far edge
MRCNN_RD_HD RleDrawBox rle_draw_box(const float* row, int h, int w)
{
    RleDrawBox b;
    b.y1 = rle_draw_round((double)row[0] * (double)(h - 1)); b.x1 = rle_draw_round((double)row[1] * (double)(w - 1));
    b.y2 = rle_draw_round((double)row[2] * (double)(h - 1) + 1.0); b.x2 = rle_draw_round((double)row[3] * (double)(w - 1) + 1.0);
    return b;
}

MRCNN_RD_HD bool rle_draw_drawn(const float* row, const RleDrawBox& b, float min_score)
{
    return row[5] > min_score && row[5] > 0.0f && b.y2 > b.y1 && b.x2 > b.x1;
}

// the stroke of a box: inside the box grown by `grow`, outside the box shrunk by `shrink` (an empty or inverted inner box contains no
// pixel: the ring is the whole outer box).  The image clips by itself: only its own pixels are asked.
MRCNN_RD_HD bool in_ring(const RleDrawBox& b, int grow, int shrink, int y, int x)
{
    const bool outer = y >= b.y1 - grow && y < b.y2 + grow && x >= b.x1 - grow && x < b.x2 + grow;
    const bool inner = y >= b.y1 + shrink && y < b.y2 - shrink && x >= b.x1 + shrink && x < b.x2 - shrink;
    return outer && !inner;
}

// palette[i % 4] of DetectionRenderer.swift:53 — red, blue, green, yellow — as one bit per channel (bit c: channel c is 255)
MRCNN_RD_HD unsigned palette_bits(int row) { return (0x3241u >> (4 * (row & 3))) & 7u; }
// what to do with a pixel that row `win` fills and row `ring` strokes (-1: none): 0 = the source, 0x10 | bits = blend the row's colour
// in, 0x20 | bits = the colour, opaque
MRCNN_RD_HD unsigned pixel_code(int win, int ring)
{
    return ring >= 0 ? 0x20u | palette_bits(ring) : (win >= 0 ? 0x10u | palette_bits(win) : 0u);
}
MRCNN_RD_HD unsigned render_byte(unsigned src, unsigned code, int ch, int alpha)
{
    const unsigned col = ((code >> ch) & 1u) * 255u;
    if (code & 0x20u) return col;
    if (code & 0x10u) return (src * (unsigned)(256 - alpha) + col * (unsigned)alpha + 128u) >> 8;
    return src;
}

}  // namespace mrcnn
