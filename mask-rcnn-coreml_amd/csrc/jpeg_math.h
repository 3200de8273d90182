// jpeg_math.h — the per-sample arithmetic of the JPEG decoder, written once for the host definition (jpeg_host.cpp, plain C++) and for
// the kernels (kernels_jpeg.hip): libjpeg's default pipeline — the "islow" inverse DCT, fancy (triangle) chroma upsampling, the 16-bit
// fixed-point YCbCr -> RGB — all in integers, so both sides produce the same bytes by construction.  No HIP header is included here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_JPEG_HD __host__ __device__ inline
#else
#define MRCNN_JPEG_HD inline
#endif

namespace mrcnn {
namespace jpeg {

enum { MODE_444 = 0, MODE_H2V1 = 1, MODE_H2V2 = 2 };

// All sums and products run in uint32_t — two's complement wrap-around, defined for ANY coefficient a damaged stream can hold; only
// the descaling shifts are arithmetic.  For encoder-made files nothing wraps and these are libjpeg's numbers.
typedef uint32_t jword;
MRCNN_JPEG_HD jword descale(jword x, int n) { return (jword)((int32_t)(x + ((jword)1 << (n - 1))) >> n); }

enum { CONST_BITS = 13, PASS1_BITS = 2 };
// FIX(x) = round(x * 2^13)
#define MRCNN_JPEG_FIX_0_298631336 2446u
#define MRCNN_JPEG_FIX_0_390180644 3196u
#define MRCNN_JPEG_FIX_0_541196100 4433u
#define MRCNN_JPEG_FIX_0_765366865 6270u
#define MRCNN_JPEG_FIX_0_899976223 7373u
#define MRCNN_JPEG_FIX_1_175875602 9633u
#define MRCNN_JPEG_FIX_1_501321110 12299u
#define MRCNN_JPEG_FIX_1_847759065 15137u
#define MRCNN_JPEG_FIX_1_961570560 16069u
#define MRCNN_JPEG_FIX_2_053119869 16819u
#define MRCNN_JPEG_FIX_2_562915447 20995u
#define MRCNN_JPEG_FIX_3_072711026 25172u

// One 1-D pass of the islow IDCT over eight values, in place.  first = true: the pass over a column of dequantised coefficients
// (descaled by CONST_BITS - PASS1_BITS); false: the pass over a row of the workspace (descaled by CONST_BITS + PASS1_BITS + 3).
MRCNN_JPEG_HD void idct_1d(jword v[8], bool first)
{
    const int shift = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
    // even part
    jword z2 = v[2], z3 = v[6];
    jword z1 = (z2 + z3) * MRCNN_JPEG_FIX_0_541196100;
    jword tmp2 = z1 - z3 * MRCNN_JPEG_FIX_1_847759065;
    jword tmp3 = z1 + z2 * MRCNN_JPEG_FIX_0_765366865;
    z2 = v[0]; z3 = v[4];
    jword tmp0 = (z2 + z3) << CONST_BITS;
    jword tmp1 = (z2 - z3) << CONST_BITS;
    const jword tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    jword z4 = tmp1 + tmp3;
    const jword z5 = (z3 + z4) * MRCNN_JPEG_FIX_1_175875602;
    tmp0 *= MRCNN_JPEG_FIX_0_298631336;
    tmp1 *= MRCNN_JPEG_FIX_2_053119869;
    tmp2 *= MRCNN_JPEG_FIX_3_072711026;
    tmp3 *= MRCNN_JPEG_FIX_1_501321110;
    z1 = (jword)0 - z1 * MRCNN_JPEG_FIX_0_899976223;
    z2 = (jword)0 - z2 * MRCNN_JPEG_FIX_2_562915447;
    z3 = (jword)0 - z3 * MRCNN_JPEG_FIX_1_961570560;
    z4 = (jword)0 - z4 * MRCNN_JPEG_FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    v[0] = descale(tmp10 + tmp3, shift); v[7] = descale(tmp10 - tmp3, shift);
    v[1] = descale(tmp11 + tmp2, shift); v[6] = descale(tmp11 - tmp2, shift);
    v[2] = descale(tmp12 + tmp1, shift); v[5] = descale(tmp12 - tmp1, shift);
    v[3] = descale(tmp13 + tmp0, shift); v[4] = descale(tmp13 - tmp0, shift);
}

MRCNN_JPEG_HD uint8_t clamp_u8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// a row pass's result -> sample: + 128, clamped
MRCNN_JPEG_HD uint8_t idct_sample(jword v) { return clamp_u8((int32_t)v + 128); }

// One chroma sample at output pixel (x, y), from the component's own plane of cw x ch REAL samples (row pitch `pitch`; what the
// padding of the block grid holds beyond them is never read).  libjpeg picks the triangle filter only where the plane is more than
// two samples wide; narrower planes are replicated.
MRCNN_JPEG_HD int32_t chroma_at(const uint8_t* plane, int64_t pitch, int cw, int ch, int x, int y, int mode)
{
    if (mode == MODE_444) return plane[(int64_t)y * pitch + x];
    const int cx = x >> 1;
    if (mode == MODE_H2V1) {
        const uint8_t* row = plane + (int64_t)y * pitch;
        const int32_t c = row[cx];
        if (cw <= 2) return c;
        if (x & 1) return cx == cw - 1 ? c : (3 * c + row[cx + 1] + 2) >> 2;
        return cx == 0 ? c : (3 * c + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = plane + (int64_t)cy * pitch;
    if (cw <= 2) return near[cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;                 // the row above for even output rows, below for odd ones; replicated at the ends
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const uint8_t* far = plane + (int64_t)fy * pitch;
    const int32_t s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

// -> R | G << 8 | B << 16
MRCNN_JPEG_HD uint32_t ycc_to_rgb(int32_t y, int32_t cb, int32_t cr)
{
    cb -= 128; cr -= 128;
    return (uint32_t)clamp_u8(y + ((91881 * cr + 32768) >> 16)) | (uint32_t)clamp_u8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16)) << 8 |
           (uint32_t)clamp_u8(y + ((116130 * cb + 32768) >> 16)) << 16;
}

// Sample planes of one image: plane[c] has pitch[c] bytes per row; chroma planes hold cw x ch real samples.
struct Planes {
    const uint8_t* plane[3];
    int64_t pitch[3];
    int ncomp, mode, cw, ch;
};
// the pixel at (x, y) as R | G << 8 | B << 16
MRCNN_JPEG_HD uint32_t pixel_rgb(const Planes& p, int x, int y)
{
    const int32_t yy = p.plane[0][(int64_t)y * p.pitch[0] + x];
    if (p.ncomp == 1) return (uint32_t)yy * 0x010101u;
    return ycc_to_rgb(yy, chroma_at(p.plane[1], p.pitch[1], p.cw, p.ch, x, y, p.mode), chroma_at(p.plane[2], p.pitch[2], p.cw, p.ch, x, y, p.mode));
}

}  // namespace jpeg
}  // namespace mrcnn
